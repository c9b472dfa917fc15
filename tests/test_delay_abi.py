"""The fourier_hip_delay_* family: include/fourier.h, the library's exports and fourier_amd._lib.DELAY_SYMBOLS name the same symbols,
every symbol resolves, the NULL-handle contract of every entry point holds, create with parameters out of range fails, and create fails
without a GPU (no compute calls: this runs without one)."""
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


def declared_delay_symbols():
    text = open(os.path.join(ROOT, "include", "fourier.h")).read()
    text = text[: text.index("Header-only C++ RAII wrapper")]
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(fourier_hip_delay_[a-z_]+_(?:float|double))\s*\(", text)))


def test_header_exports_and_binding_name_the_same_delay_symbols(libpath):
    from fourier_amd import _lib

    declared = declared_delay_symbols()
    assert len(declared) == 20 and sorted(_lib.DELAY_SYMBOLS) == declared
    out = subprocess.run(["nm", "-D", "--defined-only", libpath], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    assert sorted(s for s in exported if s.startswith("fourier_hip_delay_")) == declared
    assert set(_lib.DELAY_SYMBOLS) <= set(_lib.ALL_SYMBOLS)  # letters only: tests/test_abi.py's pattern sees them


def test_every_delay_symbol_resolves_and_the_null_handle_contract_holds_without_a_gpu(libpath):
    import ctypes

    from fourier_amd import _lib

    try:  # torch first: one HIP runtime in the process (tests/test_abi.py)
        import torch  # noqa: F401
    except Exception:
        pass
    cdll = _lib.bind(ctypes.CDLL(libpath))
    for sym in _lib.DELAY_SYMBOLS:
        assert getattr(cdll, sym) is not None
    for s in _lib.SUFFIXES:
        fn = lambda op: getattr(cdll, f"fourier_hip_delay_{op}_{s}")  # noqa: E731
        assert fn("size")(None) == 0 and fn("length")(None) == 0 and fn("channels")(None) == 0
        assert fn("describe")(None) == b""
        assert fn("last_status")(None) == INVALID
        assert fn("reserve")(None, 1) == INVALID
        assert fn("set_option")(None, b"fusion", 0) == INVALID
        assert fn("apply")(None, 16, 32, None, 64, 1, None) == INVALID
        fn("destroy")(None)
        # (size, length, channels, real_data, device): every parameter out of its range, refused before a device is looked for
        for bad in ((0, 8, 1, 1), (9, 8, 1, 1), (8, 8, 0, 1), (8, 8, 1, 2), (8, 8, 1, -1), (8, 1 << 29, 1, 1), (8, 1 << 20, 1 << 10, 0)):
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
    assert not cdll.fourier_hip_delay_create_float(1024, 2048, 1, 1, -1)
    with pytest.raises(fourier_amd.FourierError):
        fourier_amd.create_delay_f32(1024, 2048)
    with pytest.raises(fourier_amd.FourierError):
        fourier_amd.create_delay_f64(1000, 1000, real_data=False, channels=4)
    with pytest.raises(ValueError):
        fourier_amd.Delay(0, 8)
