"""The fourier_hip_czt_* family: include/fourier.h, the library's exports and fourier_amd._lib.CZT_SYMBOLS name the same symbols, every
symbol resolves, the NULL-handle contract of every entry point holds, create fails for n = 0, m = 0, w_abs = 0, parameters that are
not finite and n + m - 1 > 2^26, and create fails without a GPU (no compute calls: this runs without one)."""
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


def declared_czt_symbols():
    text = open(os.path.join(ROOT, "include", "fourier.h")).read()
    text = text[: text.index("Header-only C++ RAII wrapper")]
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(fourier_hip_czt_[a-z_]+_(?:float|double))\s*\(", text)))


def test_header_exports_and_binding_name_the_same_czt_symbols(libpath):
    from fourier_amd import _lib

    declared = declared_czt_symbols()
    assert len(declared) == 18 and sorted(_lib.CZT_SYMBOLS) == declared
    out = subprocess.run(["nm", "-D", "--defined-only", libpath], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    assert sorted(s for s in exported if s.startswith("fourier_hip_czt_")) == declared
    assert set(_lib.CZT_SYMBOLS) <= set(_lib.ALL_SYMBOLS)  # letters only: tests/test_abi.py's pattern sees them


def test_every_czt_symbol_resolves_and_the_null_handle_contract_holds_without_a_gpu(libpath):
    import ctypes

    from fourier_amd import _lib

    try:  # torch first: one HIP runtime in the process (tests/test_abi.py)
        import torch

        has_gpu = torch.cuda.is_available()
    except Exception:
        has_gpu = False
    cdll = _lib.bind(ctypes.CDLL(libpath))
    for sym in _lib.CZT_SYMBOLS:
        assert getattr(cdll, sym) is not None
    for s in _lib.SUFFIXES:
        fn = lambda op: getattr(cdll, f"fourier_hip_czt_{op}_{s}")  # noqa: E731
        assert fn("size")(None) == 0
        assert fn("points")(None) == 0
        assert fn("describe")(None) == b""
        assert fn("last_status")(None) == INVALID
        assert fn("reserve")(None, 1) == INVALID
        assert fn("set_option")(None, b"fusion", 0) == INVALID
        assert fn("transform")(None, 16, 64, 1, None) == INVALID
        fn("destroy")(None)
        create = fn("create")  # n, m, w_abs, w_turns, a_abs, a_turns, real_input, device
        assert not create(0, 8, 1.0, -0.125, 1.0, 0.0, 0, -1)
        assert not create(8, 0, 1.0, -0.125, 1.0, 0.0, 0, -1)
        assert not create(8, 8, 0.0, -0.125, 1.0, 0.0, 0, -1)
        assert not create(8, 8, 1.0, -0.125, 0.0, 0.0, 0, -1)
        for i in range(4):
            for bad in (float("nan"), float("inf")):
                pars = [1.0, -0.125, 1.0, 0.0]
                pars[i] = bad
                assert not create(8, 8, *pars, 0, -1)
        assert not create(1 << 26, 2, 1.0, -0.5, 1.0, 0.0, 0, -1)  # n + m - 1 = 2^26 + 1
    if not has_gpu:
        import fourier_amd

        assert not cdll.fourier_hip_czt_create_float(1024, 1024, 1.0, -1.0 / 1024, 1.0, 0.0, 0, -1)
        with pytest.raises(fourier_amd.FourierError):
            fourier_amd.create_czt_f32(1024, 1024)
        with pytest.raises(fourier_amd.FourierError):
            fourier_amd.create_czt_f64(100, 50, real_input=True)
