"""The fourier_hip_ipfb_* family: include/fourier.h, the library's exports and fourier_amd._lib.IPFB_SYMBOLS name the same 24 symbols,
every symbol resolves, the NULL-handle contract of every entry point holds, create fails for channels, taps or hop of 0, for
channels * taps or hop of 2^31 or more, for a real_output flag outside {0, 1}, and create fails without a GPU (no compute calls: this
runs without one)."""
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


def declared_ipfb_symbols():
    text = open(os.path.join(ROOT, "include", "fourier.h")).read()
    text = text[: text.index("Header-only C++ RAII wrapper")]
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(fourier_hip_ipfb_[a-z_]+_(?:float|double))\s*\(", text)))


def test_header_exports_and_binding_name_the_same_ipfb_symbols(libpath):
    from fourier_amd import _lib

    declared = declared_ipfb_symbols()
    assert len(declared) == 24 and sorted(_lib.IPFB_SYMBOLS) == declared
    out = subprocess.run(["nm", "-D", "--defined-only", libpath], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    assert sorted(s for s in exported if s.startswith("fourier_hip_ipfb_")) == declared
    assert set(_lib.IPFB_SYMBOLS) <= set(_lib.ALL_SYMBOLS)  # letters only: tests/test_abi.py's pattern sees them
    assert not any(s.startswith("fourier_hip_pfb_") for s in _lib.IPFB_SYMBOLS)  # a family of its own: the analysis family keeps its 26


def test_the_cxx_wrapper_names_every_entry_point():
    text = open(os.path.join(ROOT, "include", "fourier.h")).read()
    wrapper = text[text.index("template <typename T> struct ipfb;"):]
    wrapper = wrapper[: wrapper.index("#undef FOURIER_DEFINE_CXX_IPFB_WRAPPER")]
    used = set(re.findall(r"fourier_hip_ipfb_([a-z_]+)_##SUFFIX", wrapper))
    assert used == {"create", "destroy", "channels", "taps", "hop", "bins", "length", "set_filter", "inverse", "reserve", "describe",
                    "last_status"}


def test_every_ipfb_symbol_resolves_and_the_null_handle_contract_holds_without_a_gpu(libpath):
    import ctypes

    from fourier_amd import _lib

    try:  # torch first: one HIP runtime in the process (tests/test_abi.py)
        import torch

        has_gpu = torch.cuda.is_available()
    except Exception:
        has_gpu = False
    cdll = _lib.bind(ctypes.CDLL(libpath))
    for sym in _lib.IPFB_SYMBOLS:
        assert getattr(cdll, sym) is not None
    for s in _lib.SUFFIXES:
        fn = lambda op: getattr(cdll, f"fourier_hip_ipfb_{op}_{s}")  # noqa: E731
        for getter in ("channels", "taps", "hop", "bins"):
            assert fn(getter)(None) == 0
        assert fn("length")(None, 4) == 0
        assert fn("describe")(None) == b""
        assert fn("last_status")(None) == INVALID
        assert fn("reserve")(None, 4, 1) == INVALID
        assert fn("set_filter")(None, None, None) == INVALID
        assert fn("inverse")(None, 16, 4096, 4, 64, 1, None) == INVALID
        fn("destroy")(None)
        create = fn("create")  # channels, taps, hop, real_output, device
        assert not create(0, 4, 8, 0, -1)
        assert not create(8, 0, 8, 0, -1)
        assert not create(8, 4, 0, 0, -1)
        assert not create(8, 4, 8, 2, -1)
        assert not create(8, 4, 8, -1, -1)
        assert not create(1 << 16, 1 << 15, 8, 0, -1)        # channels * taps = 2^31
        assert not create(1 << 40, 1 << 40, 8, 1, -1)        # ... and where the product overflows 64 bits
        assert not create(8, 4, 1 << 31, 0, -1)              # hop above 2^31 - 1
    if not has_gpu:
        import fourier_amd

        assert not cdll.fourier_hip_ipfb_create_float(256, 4, 256, 0, -1)
        with pytest.raises(fourier_amd.FourierError):
            fourier_amd.create_ipfb_f32(256, 4)
        with pytest.raises(fourier_amd.FourierError):
            fourier_amd.create_ipfb_f64(100, 3, hop=75, real_output=True)
