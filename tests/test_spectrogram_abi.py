"""The fourier_hip_spectrogram_* family: include/fourier.h, the library's exports and fourier_amd._lib.SPECTROGRAM_SYMBOLS name the same
symbols, the NULL-handle contract of every entry point holds, the enum agrees with the Python table, and create fails without a GPU (no
compute calls: this runs without one)."""
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


def declared_spectrogram_symbols():
    text = open(os.path.join(ROOT, "include", "fourier.h")).read()
    text = text[: text.index("Header-only C++ RAII wrapper")]
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(fourier_hip_spectrogram_[a-z_]+_(?:float|double))\s*\(", text)))


def test_header_exports_and_binding_name_the_same_spectrogram_symbols(libpath):
    from fourier_amd import _lib

    declared = declared_spectrogram_symbols()
    assert len(declared) == 28 and sorted(_lib.SPECTROGRAM_SYMBOLS) == declared
    out = subprocess.run(["nm", "-D", "--defined-only", libpath], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    assert sorted(s for s in exported if s.startswith("fourier_hip_spectrogram_")) == declared
    assert set(_lib.SPECTROGRAM_SYMBOLS) <= set(_lib.ALL_SYMBOLS)  # letters only: tests/test_abi.py's pattern sees them


def test_every_spectrogram_symbol_resolves_and_the_null_handle_contract_holds_without_a_gpu(libpath):
    import ctypes

    from fourier_amd import _lib

    try:  # torch first: one HIP runtime in the process (tests/test_abi.py)
        import torch

        has_gpu = torch.cuda.is_available()
    except Exception:
        has_gpu = False
    cdll = _lib.bind(ctypes.CDLL(libpath))
    for sym in _lib.SPECTROGRAM_SYMBOLS:
        assert getattr(cdll, sym) is not None
    for s in _lib.SUFFIXES:
        fn = lambda op: getattr(cdll, f"fourier_hip_spectrogram_{op}_{s}")  # noqa: E731
        for getter in ("n_fft", "hop", "win_length", "bins"):
            assert fn(getter)(None) == 0
        assert fn("frames")(None, 100) == 0
        assert fn("describe")(None) == b""
        assert fn("last_status")(None) == INVALID
        assert fn("reserve")(None, 100, 1) == INVALID
        assert fn("set_window")(None, 16, None) == INVALID
        assert fn("set_option")(None, b"fusion", 0) == INVALID
        assert fn("forward")(None, 16, 32, 100, 1, 2, 0, None) == INVALID
        assert fn("welch")(None, 16, 32, 100, 1, 1, 1.0, None) == INVALID
        fn("destroy")(None)
        for bad in ((0, 1, 1, 1), (8, 0, 8, 1), (8, 2, 9, 1), (8, 2, 8, 3)):
            assert not fn("create")(*bad, -1)
    if not has_gpu:
        import fourier_amd

        assert not cdll.fourier_hip_spectrogram_create_float(256, 64, 256, 1, -1)
        with pytest.raises(fourier_amd.FourierError):
            fourier_amd.create_spectrogram_f32(256)
        with pytest.raises(fourier_amd.FourierError):
            fourier_amd.create_spectrogram_f64(400, 160, center=False)


def test_enum_of_the_header_matches_the_python_table():
    from fourier_amd import fft

    text = open(os.path.join(ROOT, "include", "fourier.h")).read()
    values = {m.group(1): int(m.group(2)) for m in re.finditer(r"\b(FOURIER_SPECTROGRAM_[A-Z_]+) = (\d+),", text)}
    assert values == {"FOURIER_SPECTROGRAM_MAGNITUDE": 1, "FOURIER_SPECTROGRAM_POWER": 2}
    assert fft.SPECTROGRAM_POWERS == {"magnitude": 1, "power": 2}
