"""The fourier_hip_csd_* family: include/fourier.h, the library's exports and fourier_amd._lib.CSD_SYMBOLS name the same symbols, every
symbol resolves, the NULL-handle contract of every entry point holds, and create fails without a GPU (no compute calls: this runs
without one)."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = 1


@pytest.fixture(scope="module")
def libpath():
    from fourier_amd import build

    return build.build()


def declared_csd_symbols():
    text = open(os.path.join(ROOT, "include", "fourier.h")).read()
    text = text[: text.index("Header-only C++ RAII wrapper")]
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(fourier_hip_csd_[a-z_]+_(?:float|double))\s*\(", text)))


def test_header_exports_and_binding_name_the_same_csd_symbols(libpath):
    from fourier_amd import _lib

    declared = declared_csd_symbols()
    assert len(declared) == 28 and sorted(_lib.CSD_SYMBOLS) == declared
    out = subprocess.run(["nm", "-D", "--defined-only", libpath], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    assert sorted(s for s in exported if s.startswith("fourier_hip_csd_")) == declared
    assert set(_lib.CSD_SYMBOLS) <= set(_lib.ALL_SYMBOLS)  # letters only: tests/test_abi.py's pattern sees them


def test_every_csd_symbol_resolves_and_the_null_handle_contract_holds_without_a_gpu(libpath):
    import ctypes

    from fourier_amd import _lib

    try:  # torch first: one HIP runtime in the process (tests/test_abi.py)
        import torch

        has_gpu = torch.cuda.is_available()
    except Exception:
        has_gpu = False
    cdll = _lib.bind(ctypes.CDLL(libpath))
    for sym in _lib.CSD_SYMBOLS:
        assert getattr(cdll, sym) is not None
    for s in _lib.SUFFIXES:
        fn = lambda op: getattr(cdll, f"fourier_hip_csd_{op}_{s}")  # noqa: E731
        for getter in ("n_fft", "hop", "win_length", "bins"):
            assert fn(getter)(None) == 0
        assert fn("frames")(None, 100) == 0
        assert fn("describe")(None) == b""
        assert fn("last_status")(None) == INVALID
        assert fn("reserve")(None, 100, 1) == INVALID
        assert fn("set_window")(None, 16, None) == INVALID
        assert fn("set_option")(None, b"fusion", 0) == INVALID
        assert fn("csd")(None, 16, 32, 64, 100, 1, 1, 1.0, None) == INVALID
        assert fn("coherence")(None, 16, 32, 64, 100, 1, None) == INVALID
        fn("destroy")(None)
        for bad in ((0, 1, 1, 1), (8, 0, 8, 1), (8, 2, 9, 1), (8, 2, 8, 3)):
            assert not fn("create")(*bad, -1)
    if not has_gpu:
        import fourier_amd

        assert not cdll.fourier_hip_csd_create_float(256, 64, 256, 1, -1)
        with pytest.raises(fourier_amd.FourierError):
            fourier_amd.create_csd_f32(256)
        with pytest.raises(fourier_amd.FourierError):
            fourier_amd.create_csd_f64(400, 160, center=False)
