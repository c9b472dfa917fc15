"""The fourier_hip_r2r_* family: include/fourier.h, the library's exports and fourier_amd._lib.R2R_SYMBOLS name the same symbols
(no compute calls: this runs without a GPU).  tests/test_abi.py holds this check for the other families; its pattern admits letters
only, so it does not see names with a digit."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def libpath():
    from fourier_amd import build

    return build.build()


def declared_r2r_symbols():
    text = open(os.path.join(ROOT, "include", "fourier.h")).read()
    text = text[: text.index("Header-only C++ RAII wrapper")]
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(fourier_hip_r2r_[a-z_]+_(?:float|double))\s*\(", text)))


def test_header_exports_and_binding_name_the_same_r2r_symbols(libpath):
    from fourier_amd import _lib

    declared = declared_r2r_symbols()
    assert len(declared) == 14 and sorted(_lib.R2R_SYMBOLS) == declared
    out = subprocess.run(["nm", "-D", "--defined-only", libpath], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    assert [s for s in declared if s not in exported] == []
    assert sorted(s for s in exported if s.startswith("fourier_hip_r2r_")) == declared
    assert not set(_lib.R2R_SYMBOLS) & set(_lib.ALL_SYMBOLS)


def test_every_r2r_symbol_resolves_and_the_null_handle_contract_holds_without_a_gpu(libpath):
    import ctypes

    from fourier_amd import _lib

    try:  # torch first: one HIP runtime in the process (tests/test_abi.py)
        import torch

        has_gpu = torch.cuda.is_available()
    except Exception:
        has_gpu = False
    cdll = _lib.bind(ctypes.CDLL(libpath))
    for sym in _lib.R2R_SYMBOLS:
        assert getattr(cdll, sym) is not None
    for s in _lib.SUFFIXES:
        assert getattr(cdll, f"fourier_hip_r2r_size_{s}")(None) == 0
        assert getattr(cdll, f"fourier_hip_r2r_describe_{s}")(None) == b""
        assert getattr(cdll, f"fourier_hip_r2r_last_status_{s}")(None) == 1
        assert getattr(cdll, f"fourier_hip_r2r_reserve_{s}")(None, 1) == 1
        assert getattr(cdll, f"fourier_hip_r2r_transform_batch_{s}")(None, 16, 16, 1, 0, 0, None) == 1
        getattr(cdll, f"fourier_hip_r2r_destroy_{s}")(None)
        assert not getattr(cdll, f"fourier_hip_r2r_create_{s}")(0, -1)
    if not has_gpu:
        import fourier_amd

        assert not cdll.fourier_hip_r2r_create_float(8, -1)
        with pytest.raises(fourier_amd.FourierError):
            fourier_amd.create_r2r_f32(8)


def test_enums_of_the_header_match_the_python_tables():
    from fourier_amd import fft

    text = open(os.path.join(ROOT, "include", "fourier.h")).read()
    values = {m.group(1): int(m.group(2)) for m in re.finditer(r"\b(FOURIER_R2R_[A-Z0-9_]+) = (\d+),", text)}
    assert values == {"FOURIER_R2R_DCT2": 0, "FOURIER_R2R_DCT3": 1, "FOURIER_R2R_DST2": 2, "FOURIER_R2R_DST3": 3,
                      "FOURIER_R2R_NORM_BACKWARD": 0, "FOURIER_R2R_NORM_ORTHO": 1, "FOURIER_R2R_NORM_FORWARD": 2}
    assert fft.R2R_KINDS == {("dct", 2): 0, ("dct", 3): 1, ("dst", 2): 2, ("dst", 3): 3}
    assert fft.R2R_NORMS == {None: 0, "backward": 0, "ortho": 1, "forward": 2}
