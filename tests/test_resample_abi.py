"""The fourier_hip_resample_* family: include/fourier.h, the library's exports and fourier_amd._lib.RESAMPLE_SYMBOLS name the same
symbols, every symbol resolves, the NULL-handle contract of every entry point holds, create with a length of 0 fails, and create fails
without a GPU (no compute calls on the product library: this runs without one).  The argument checks that need a live handle -- overlap,
misaligned complex buffers, a bad option key or value -- run on the emulator build (tests/emu)."""
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = 1


@pytest.fixture(scope="module")
def libpath():
    from fourier_amd import build

    return build.build()


def declared_resample_symbols():
    text = open(os.path.join(ROOT, "include", "fourier.h")).read()
    text = text[: text.index("Header-only C++ RAII wrapper")]
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(fourier_hip_resample_[a-z_]+_(?:float|double))\s*\(", text)))


def test_header_exports_and_binding_name_the_same_resample_symbols(libpath):
    from fourier_amd import _lib

    declared = declared_resample_symbols()
    assert len(declared) == 22 and sorted(_lib.RESAMPLE_SYMBOLS) == declared
    out = subprocess.run(["nm", "-D", "--defined-only", libpath], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    assert sorted(s for s in exported if s.startswith("fourier_hip_resample_")) == declared
    assert set(_lib.RESAMPLE_SYMBOLS) <= set(_lib.ALL_SYMBOLS)  # letters only: tests/test_abi.py's pattern sees them


def test_every_resample_symbol_resolves_and_the_null_handle_contract_holds_without_a_gpu(libpath):
    import ctypes

    from fourier_amd import _lib

    try:  # torch first: one HIP runtime in the process (tests/test_abi.py)
        import torch

        has_gpu = torch.cuda.is_available()
    except Exception:
        has_gpu = False
    cdll = _lib.bind(ctypes.CDLL(libpath))
    for sym in _lib.RESAMPLE_SYMBOLS:
        assert getattr(cdll, sym) is not None
    for s in _lib.SUFFIXES:
        fn = lambda op: getattr(cdll, f"fourier_hip_resample_{op}_{s}")  # noqa: E731
        assert fn("size_in")(None) == 0 and fn("size_out")(None) == 0 and fn("real_input")(None) == 0
        assert fn("describe")(None) == b""
        assert fn("last_status")(None) == INVALID
        assert fn("reserve")(None, 1) == INVALID
        assert fn("set_option")(None, b"fusion", 0) == INVALID
        assert fn("set_window")(None, None, None) == INVALID
        assert fn("forward")(None, 16, 64, 1, None) == INVALID
        fn("destroy")(None)
        for real_input in (0, 1):
            assert not fn("create")(0, 8, real_input, -1)
            assert not fn("create")(8, 0, real_input, -1)
    if not has_gpu:
        import fourier_amd

        assert not cdll.fourier_hip_resample_create_float(2048, 1024, 1, -1)
        with pytest.raises(fourier_amd.FourierError):
            fourier_amd.create_resample_f32(2048, 1024)
        with pytest.raises(fourier_amd.FourierError):
            fourier_amd.create_resample_f64(1000, 1031, real_input=False)


@pytest.fixture
def fa():
    from emu import build_emu
    from fourier_amd import _lib

    prev = _lib._lib
    _lib._lib = build_emu.load()  # a live handle without a GPU: the emulation build behind the same C ABI
    import fourier_amd

    yield fourier_amd
    _lib._lib = prev


def test_argument_checks_of_a_live_handle(fa):
    from fourier_amd import _lib

    L = _lib.lib()
    fn = lambda op: getattr(L, f"fourier_hip_resample_{op}_double")  # noqa: E731
    create, fwd, status, opt, reserve, setw = (fn(op) for op in ("create", "forward", "last_status", "set_option", "reserve", "set_window"))
    for real_input in (0, 1):
        assert not create(0, 8, real_input, -1) and not create(8, 0, real_input, -1)
    assert not create(8, 8, 2, -1)  # the flag is 0 or 1
    n, m = 16, 12
    big = np.zeros(64 * n)
    B = big.ctypes.data
    # real rows: 8-byte values, any value boundary
    plan = fa.Resample(n, m, "f64")
    h = plan._h
    assert fn("size_in")(h) == n and fn("size_out")(h) == m and fn("real_input")(h) == 1
    x, y = np.zeros((2, n)), np.zeros((2, m))
    X, Y = x.ctypes.data, y.ctypes.data
    assert fwd(h, X, Y, 2, None) == 0 and status(h) == 0
    assert fwd(h, None, Y, 2, None) == INVALID and status(h) == INVALID
    assert fwd(h, X, None, 2, None) == INVALID
    assert fwd(h, X + 4, Y, 1, None) == INVALID and fwd(h, X, Y + 4, 1, None) == INVALID
    assert fwd(h, X + 8, Y + 8, 1, None) == 0                    # an odd real is enough on both sides
    assert fwd(h, B, B, 2, None) == INVALID                      # never in place
    assert fwd(h, B, B + 2 * n * 8, 2, None) == 0                # the output behind the input: adjacent
    assert fwd(h, B, B + 2 * n * 8 - 8, 2, None) == INVALID      # ... one real earlier: inside it
    assert fwd(h, B + 2 * m * 8, B, 2, None) == 0                # the input behind the output: adjacent
    assert fwd(h, B + 2 * m * 8 - 8, B, 2, None) == INVALID
    assert fwd(h, X, Y, 0, None) == 0                            # batch 0: a no-op
    assert reserve(h, 0) == 0 and reserve(h, 2) == 0
    assert opt(h, b"fusion", 2) == INVALID and opt(h, b"fusion", -1) == INVALID
    assert opt(h, b"no_such_option", 1) == INVALID and opt(h, None, 1) == INVALID
    assert opt(h, b"fusion", 1) == 0 and plan.describe().startswith("resample real fused untangle: ")
    assert opt(h, b"fusion", 0) == 0 and plan.describe().startswith("resample real composed: ")
    assert setw(h, B + 4, None) == INVALID and setw(h, B, None) == 0 and setw(h, None, None) == 0
    # complex rows: 16-byte values
    plan = fa.Resample(n, m, "f64", real_input=False)
    h = plan._h
    assert fn("real_input")(h) == 0 and plan.describe().startswith("resample complex: ")
    x, y = np.zeros((2, n), np.complex128), np.zeros((2, m), np.complex128)
    X, Y = x.ctypes.data, y.ctypes.data
    assert fwd(h, X, Y, 2, None) == 0
    assert fwd(h, X + 8, Y, 1, None) == INVALID and fwd(h, X, Y + 8, 1, None) == INVALID   # misaligned complex buffers
    assert fwd(h, X + 16, Y + 16, 1, None) == 0
    assert fwd(h, B, B, 2, None) == INVALID
    assert fwd(h, B, B + 2 * n * 16, 2, None) == 0 and fwd(h, B, B + 2 * n * 16 - 16, 2, None) == INVALID
    assert opt(h, b"fusion", 1) == 0 and opt(h, b"fusion", 0) == 0 and plan.describe().startswith("resample complex: ")
    assert opt(h, b"fusion", 2) == INVALID
    with pytest.raises(fa.FourierError):
        plan.forward_ptr(0, Y, 1)
    with pytest.raises(ValueError):
        fa.Resample(0, 4, "f32")
    with pytest.raises(ValueError):
        fa.Resample(4, 0, "f32")
