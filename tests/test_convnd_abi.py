"""The fourier_hip_convnd_* family: include/fourier.h, the library's exports and fourier_amd._lib.CONVND_SYMBOLS name the same
symbols -- create, destroy, rank, shape, filters, set_filters, set_window, apply_batch, reserve, set_option, describe and last_status,
for float and double --, every symbol resolves, the NULL-handle contract of every entry point holds, create with a rank or a shape out
of range fails before a device is looked for, and create fails without a GPU (no compute calls: this runs without one).  The argument
checks that need a handle run on the emulator build (tests/test_convnd_emu.py) and on the GPU (tests/test_gpu_convnd.py)."""
import ctypes
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = 1
OPS = ("create", "destroy", "rank", "shape", "filters", "set_filters", "set_window", "apply_batch", "reserve", "set_option", "describe",
       "last_status")


@pytest.fixture(scope="module")
def libpath():
    from fourier_amd import build

    return build.build()


def declared_convnd_symbols():
    text = open(os.path.join(ROOT, "include", "fourier.h")).read()
    text = text[: text.index("Header-only C++ RAII wrapper")]
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(fourier_hip_convnd_[a-z_]+_(?:float|double))\s*\(", text)))


def sizes(*v):
    return (ctypes.c_size_t * len(v))(*v)


def test_header_exports_and_binding_name_the_same_convnd_symbols(libpath):
    from fourier_amd import _lib

    declared = declared_convnd_symbols()
    assert declared == sorted(f"fourier_hip_convnd_{op}_{s}" for op in OPS for s in ("float", "double"))
    assert sorted(_lib.CONVND_SYMBOLS) == declared
    out = subprocess.run(["nm", "-D", "--defined-only", libpath], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    assert sorted(s for s in exported if s.startswith("fourier_hip_convnd_")) == declared
    assert set(_lib.CONVND_SYMBOLS) <= set(_lib.ALL_SYMBOLS)  # letters only: tests/test_abi.py's pattern sees them


def test_the_cxx_wrapper_and_the_cmake_package_name_the_family():
    text = open(os.path.join(ROOT, "include", "fourier.h")).read()
    wrapper = text[text.index("Header-only C++ RAII wrapper"):]
    assert "template <typename T> struct convnd;" in wrapper
    for op in OPS:
        assert f"fourier_hip_convnd_{op}_##SUFFIX" in wrapper, op
    assert re.search(r"foreach\(FAMILY [^)]*\bconvnd\b", open(os.path.join(ROOT, "packaging", "CMakeLists.txt")).read())


def test_every_convnd_symbol_resolves_and_the_null_handle_contract_holds_without_a_gpu(libpath):
    from fourier_amd import _lib

    try:  # torch first: one HIP runtime in the process (tests/test_abi.py)
        import torch  # noqa: F401
    except Exception:
        pass
    cdll = _lib.bind(ctypes.CDLL(libpath))
    for sym in _lib.CONVND_SYMBOLS:
        assert getattr(cdll, sym) is not None
    three = sizes(2, 3, 4)
    for s in _lib.SUFFIXES:
        fn = lambda op: getattr(cdll, f"fourier_hip_convnd_{op}_{s}")  # noqa: E731
        assert fn("rank")(None) == 0 and fn("filters")(None) == 0
        assert fn("shape")(None, three) == INVALID
        assert fn("describe")(None) == b""
        assert fn("last_status")(None) == INVALID
        assert fn("reserve")(None, 1) == INVALID
        assert fn("set_option")(None, b"fusion", 0) == INVALID
        assert fn("set_filters")(None, 16, three, 1, 0, None) == INVALID
        assert fn("set_window")(None, three, three, three) == INVALID
        assert fn("apply_batch")(None, 16, 64, 1, 0, None) == INVALID
        fn("destroy")(None)
        # refused before a device is looked for: rank 1 (fourier_hip_conv_*), rank 5, rank 0, a NULL shape, a length of 0, an item too large
        for rank, shape in ((1, sizes(16)), (5, sizes(2, 2, 2, 2, 2)), (0, sizes(2)), (-1, sizes(2)), (2, None), (2, sizes(4, 0)),
                            (3, sizes(0, 4, 4)), (2, sizes(1 << 33, 8)), (2, sizes(1 << 40, 1 << 40))):
            assert not fn("create")(rank, shape, -1), (rank, shape and list(shape))


def test_create_fails_without_a_gpu(libpath):
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
    assert not cdll.fourier_hip_convnd_create_float(2, sizes(64, 64), -1)
    with pytest.raises(fourier_amd.FourierError):
        fourier_amd.create_convnd_f32((64, 64))
    with pytest.raises(fourier_amd.FourierError):
        fourier_amd.create_convnd_f64((3, 5, 9))
    with pytest.raises(ValueError):
        fourier_amd.FftConvNd((16,), "f32")
