"""The fourier_hip_bandspec_* family: include/fourier.h, the library's exports and fourier_amd._lib.BANDSPEC_SYMBOLS name the same 30
symbols, every symbol resolves, the NULL-handle contract of every entry point holds, create fails for bands of 0 and above 65535 and
for parameters outside the STFT handle's ranges, and create fails without a GPU (no compute calls: this runs without one)."""
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


def declared_bandspec_symbols():
    text = open(os.path.join(ROOT, "include", "fourier.h")).read()
    text = text[: text.index("Header-only C++ RAII wrapper")]
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(fourier_hip_bandspec_[a-z_]+_(?:float|double))\s*\(", text)))


def test_header_exports_and_binding_name_the_same_bandspec_symbols(libpath):
    from fourier_amd import _lib

    declared = declared_bandspec_symbols()
    assert len(declared) == 30 and sorted(_lib.BANDSPEC_SYMBOLS) == declared
    out = subprocess.run(["nm", "-D", "--defined-only", libpath], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    assert sorted(s for s in exported if s.startswith("fourier_hip_bandspec_")) == declared
    assert set(_lib.BANDSPEC_SYMBOLS) <= set(_lib.ALL_SYMBOLS)  # letters only: tests/test_abi.py's pattern sees them
    assert not any(s.startswith("fourier_hip_spectrogram_") for s in _lib.BANDSPEC_SYMBOLS)  # a family of its own: the spectrogram keeps its 28
    assert len(_lib.SPECTROGRAM_SYMBOLS) == 28


def test_the_cxx_wrapper_names_every_entry_point():
    text = open(os.path.join(ROOT, "include", "fourier.h")).read()
    wrapper = text[text.index("template <typename T> struct bandspec;"):]
    wrapper = wrapper[: wrapper.index("#undef FOURIER_DEFINE_CXX_BANDSPEC_WRAPPER")]
    used = set(re.findall(r"fourier_hip_bandspec_([a-z_]+)_##SUFFIX", wrapper))
    assert used == {"create", "destroy", "n_fft", "hop", "win_length", "bins", "bands", "frames", "set_window", "set_bands", "forward",
                    "reserve", "set_option", "describe", "last_status"}


def test_every_bandspec_symbol_resolves_and_the_null_handle_contract_holds_without_a_gpu(libpath):
    import ctypes

    from fourier_amd import _lib

    try:  # torch first: one HIP runtime in the process (tests/test_abi.py)
        import torch

        has_gpu = torch.cuda.is_available()
    except Exception:
        has_gpu = False
    cdll = _lib.bind(ctypes.CDLL(libpath))
    for sym in _lib.BANDSPEC_SYMBOLS:
        assert getattr(cdll, sym) is not None
    for s in _lib.SUFFIXES:
        fn = lambda op: getattr(cdll, f"fourier_hip_bandspec_{op}_{s}")  # noqa: E731
        for getter in ("n_fft", "hop", "win_length", "bins", "bands"):
            assert fn(getter)(None) == 0
        assert fn("frames")(None, 4096) == 0
        assert fn("describe")(None) == b""
        assert fn("last_status")(None) == INVALID
        assert fn("reserve")(None, 4096, 1) == INVALID
        assert fn("set_window")(None, None, None) == INVALID
        assert fn("set_bands")(None, None, None) == INVALID
        assert fn("set_option")(None, b"fusion", 1) == INVALID
        assert fn("forward")(None, 16, 4096, 1024, 1, 2, 0, 0.0, 0.0, None) == INVALID
        fn("destroy")(None)
        create = fn("create")  # n_fft, hop, win_length, pad_mode, bands, device
        assert not create(256, 64, 256, 1, 0, -1)              # bands = 0
        assert not create(256, 64, 256, 1, 65536, -1)          # bands above 65535
        assert not create(256, 64, 256, 1, 1 << 40, -1)
        assert not create(0, 64, 1, 1, 40, -1)                 # the STFT handle's ranges
        assert not create(256, 0, 256, 1, 40, -1)
        assert not create(256, 64, 257, 1, 40, -1)
        assert not create(256, 64, 256, 3, 40, -1)
    if not has_gpu:
        import fourier_amd

        assert not cdll.fourier_hip_bandspec_create_float(256, 64, 256, 1, 40, -1)
        assert not cdll.fourier_hip_bandspec_create_double(256, 64, 256, 1, 65535, -1)
        with pytest.raises(fourier_amd.FourierError):
            fourier_amd.create_bandspec_f32(256, 40)
        with pytest.raises(fourier_amd.FourierError):
            fourier_amd.create_bandspec_f64(400, 40, hop_length=160)
        with pytest.raises(ValueError):
            fourier_amd.create_bandspec_f32(256, 0)
        with pytest.raises(ValueError):
            fourier_amd.create_bandspec_f32(256, 65536)
