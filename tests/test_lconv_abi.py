"""The linear-convolution family of the C ABI (fourier_hip_lconv_*) without a GPU: the header, the library's exports and the
Python binding name the same 24 symbols, the NULL-handle contract holds, the mode enum matches the Python table, and create refuses
what include/fourier.h says it refuses (without a device every create fails; the emulator twin, tests/test_lconv_emu.py, creates)."""
import ctypes
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = 1  # FOURIER_HIP_INVALID_ARGUMENT
OPS = ("create", "destroy", "length", "taps", "out_length", "filters", "set_filters", "apply", "reserve", "set_option", "describe",
       "last_status")


@pytest.fixture(scope="module")
def libpath():
    from fourier_amd import build

    return build.build()


def header():
    text = open(os.path.join(ROOT, "include", "fourier.h")).read()
    text = text[: text.index("Header-only C++ RAII wrapper")]
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def test_header_exports_and_binding_name_the_same_24_symbols(libpath):
    from fourier_amd import _lib

    expected = sorted(f"fourier_hip_lconv_{op}_{s}" for op in OPS for s in ("float", "double"))
    assert len(expected) == 24
    declared = sorted(set(re.findall(r"\b(fourier_hip_lconv_[a-z_]+_(?:float|double))\s*\(", header())))
    assert declared == expected
    assert sorted(_lib.LCONV_SYMBOLS) == expected and set(expected) <= set(_lib.ALL_SYMBOLS)
    out = subprocess.run(["nm", "-D", "--defined-only", libpath], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    assert sorted(s for s in exported if s.startswith("fourier_hip_lconv_")) == expected


def test_mode_enum_matches_the_python_table():
    from fourier_amd import fft

    body = re.search(r"enum fourier_lconv_mode \{(.*?)\}", header(), re.S).group(1)
    values = {name.lower(): int(v) for name, v in re.findall(r"FOURIER_LCONV_([A-Z]+) = (\d+)", body)}
    assert values == {"full": 0, "same": 1, "valid": 2} == fft.LCONV_MODES


def test_null_handle_contract_and_refused_creates(libpath):
    try:  # torch first: one HIP runtime in the process (tests/test_abi.py)
        import torch  # noqa: F401
    except Exception:
        pass
    from fourier_amd import _lib

    L = _lib.bind(ctypes.CDLL(libpath))
    for s in ("float", "double"):
        f = lambda op: getattr(L, f"fourier_hip_lconv_{op}_{s}")  # noqa: E731
        assert f("length")(None) == 0 and f("taps")(None) == 0 and f("out_length")(None) == 0 and f("filters")(None) == 0
        assert f("describe")(None) == b""
        assert f("last_status")(None) == INVALID
        assert f("apply")(None, 16, 32, 1, None) == INVALID
        assert f("set_filters")(None, 16, 1, 0, None) == INVALID
        assert f("reserve")(None, 1) == INVALID
        assert f("set_option")(None, b"block", 0) == INVALID
        f("destroy")(None)
        for real_data in (0, 1):
            assert not f("create")(0, 5, 0, real_data, -1)      # length == 0
            assert not f("create")(100, 0, 0, real_data, -1)    # taps == 0
            assert not f("create")(100, 5, 3, real_data, -1)    # an unknown mode
            assert not f("create")(100, 5, -1, real_data, -1)
            assert not f("create")(4, 5, 2, real_data, -1)      # VALID with K > Lx


def test_python_layer_refuses_an_unknown_mode():
    import fourier_amd

    with pytest.raises(ValueError):
        fourier_amd.LinearConv(100, 5, "f32", "causal")
