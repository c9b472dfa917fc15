"""The fourier_hip_cepstrum_* family: include/fourier.h, the library's exports and fourier_amd._lib.CEPSTRUM_SYMBOLS name the same
symbols -- create, destroy, size, length, outputs, mode, apply, reserve, set_option, describe and the last_status that every handle
family has, for float and double --, every symbol resolves, the NULL-handle contract of every entry point holds, create with
parameters out of range fails, and create fails without a GPU (no compute calls: this runs without one).  The per-call reals that
are refused AFTER rounding to the handle's precision are checked on the CPU emulation build (tests/emu), where a handle exists."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = 1
OPS = ("create", "destroy", "size", "length", "outputs", "mode", "apply", "reserve", "set_option", "describe", "last_status")


@pytest.fixture(scope="module")
def libpath():
    from fourier_amd import build

    return build.build()


def declared_cepstrum_symbols():
    text = open(os.path.join(ROOT, "include", "fourier.h")).read()
    text = text[: text.index("Header-only C++ RAII wrapper")]
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(fourier_hip_cepstrum_[a-z_]+_(?:float|double))\s*\(", text)))


def test_header_exports_and_binding_name_the_same_cepstrum_symbols(libpath):
    from fourier_amd import _lib

    declared = declared_cepstrum_symbols()
    assert declared == sorted(f"fourier_hip_cepstrum_{op}_{s}" for op in OPS for s in ("float", "double"))
    assert sorted(_lib.CEPSTRUM_SYMBOLS) == declared
    out = subprocess.run(["nm", "-D", "--defined-only", libpath], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    assert sorted(s for s in exported if s.startswith("fourier_hip_cepstrum_")) == declared
    assert set(_lib.CEPSTRUM_SYMBOLS) <= set(_lib.ALL_SYMBOLS)  # letters only: tests/test_abi.py's pattern sees them


def test_every_cepstrum_symbol_resolves_and_the_null_handle_contract_holds_without_a_gpu(libpath):
    import ctypes

    from fourier_amd import _lib

    try:  # torch first: one HIP runtime in the process (tests/test_abi.py)
        import torch  # noqa: F401
    except Exception:
        pass
    cdll = _lib.bind(ctypes.CDLL(libpath))
    for sym in _lib.CEPSTRUM_SYMBOLS:
        assert getattr(cdll, sym) is not None
    for s in _lib.SUFFIXES:
        fn = lambda op: getattr(cdll, f"fourier_hip_cepstrum_{op}_{s}")  # noqa: E731
        assert fn("size")(None) == 0 and fn("length")(None) == 0 and fn("outputs")(None) == 0 and fn("mode")(None) == -1
        assert fn("describe")(None) == b""
        assert fn("last_status")(None) == INVALID
        assert fn("reserve")(None, 1) == INVALID
        assert fn("set_option")(None, b"fusion", 0) == INVALID
        assert fn("apply")(None, 16, 64, 1, 1.0, 0.0, None) == INVALID
        fn("destroy")(None)
        # (size, length, outputs, mode, device): every parameter out of its range, refused before a device is looked for
        for bad in ((0, 8, 1, 0), (9, 8, 1, 0), (8, 8, 0, 0), (8, 8, 9, 0), (8, 8, 8, 2), (8, 8, 8, -1), (8, 1 << 29, 8, 1)):
            assert not fn("create")(*bad, -1), bad


def test_create_fails_without_a_gpu(libpath):
    import ctypes

    from fourier_amd import _lib

    try:
        import torch

        has_gpu = torch.cuda.is_available()
    except Exception:
        has_gpu = False
    if has_gpu:
        return  # the GPU tests create handles
    import fourier_amd

    cdll = _lib.bind(ctypes.CDLL(libpath))
    assert not cdll.fourier_hip_cepstrum_create_float(1024, 2048, 1024, 0, -1)
    with pytest.raises(fourier_amd.FourierError):
        fourier_amd.create_cepstrum_f32(1024, 2048)
    with pytest.raises(fourier_amd.FourierError):
        fourier_amd.create_cepstrum_f64(1000, 1000, 500, mode=1)
    with pytest.raises(ValueError):
        fourier_amd.Cepstrum(0, 8)


def test_parameters_that_round_out_of_range_in_float_are_refused_and_write_nothing():
    """log_floor > 0 that rounds to 0 (1e-200), to a subnormal (1e-40) or to inf (1e39) in float, and log_mult that rounds to 0 (1e-50)
    or to inf (1e60): FOURIER_HIP_INVALID_ARGUMENT from the call and from last_status, and the output keeps every byte.  The same
    values are valid for the double handle.  (Before the check: 1e-200 was taken as "no floor", 1e-50 returned zeros and 1e60 NaN,
    all with status success.)"""
    import numpy as np

    from emu import build_emu

    lib = build_emu.load()
    n, L, batch = 600, 1000, 3
    x = np.ones((batch, n), np.float32)
    x[:, 1:] = 0.01
    for suffix, dt, refused in (("float", np.float32, True), ("double", np.float64, False)):
        fn = lambda op: getattr(lib, f"fourier_hip_cepstrum_{op}_{suffix}")  # noqa: E731
        for mode in (0, 1):
            h = fn("create")(n, L, n, mode, -1)
            assert h
            xin = np.ascontiguousarray(x.astype(dt))
            try:
                for fusion in (1, 0):
                    assert fn("set_option")(h, b"fusion", fusion) == 0
                    for log_mult, log_floor in ((1.0, 1e-200), (1.0, 1e-40), (1.0, 1e39), (1e-50, 0.0), (1e60, 0.0), (-1e-50, 1e-3), (-1e60, 1e-3)):
                        out = np.full((batch, n), 77.0, dt)
                        st = fn("apply")(h, xin.ctypes.data, out.ctypes.data, batch, log_mult, log_floor, None)
                        if refused:
                            assert st == INVALID and fn("last_status")(h) == INVALID, (suffix, mode, log_mult, log_floor, st)
                            assert np.all(out == 77.0), (suffix, mode, log_mult, log_floor, "the output was written")
                        else:
                            assert st == 0 and fn("last_status")(h) == 0, (suffix, mode, log_mult, log_floor, st)
                    assert fn("apply")(h, xin.ctypes.data, out.ctypes.data, batch, 1.0, 0.0, None) == 0 and fn("last_status")(h) == 0
            finally:
                fn("destroy")(h)
