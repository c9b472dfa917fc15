"""The fourier_hip_nufft3d_* family: include/fourier.h, the library's exports and fourier_amd._lib.NUFFT3D_SYMBOLS name the same 26
symbols -- create, destroy, modes1, modes2, modes3, points, set_points, to_modes_batch, to_points_batch, reserve, set_option, describe
and last_status, for float and double --, every symbol resolves, the NULL-handle contract of every entry point holds, create with a
parameter out of range fails before a device is looked for, and create fails without a GPU (no compute calls: this runs without one).
The family is listed apart from _lib.ALL_SYMBOLS, as the 2-D family is: tests/test_abi.py compares that list with the names a
letters-only pattern finds in the header, and the pattern cannot see "nufft3d".  The argument checks that need a handle run on the
emulator build (tests/test_nufft3d_emu.py) and on the GPU (tests/test_gpu_nufft3d.py)."""
import ctypes
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = 1
OPS = ("create", "destroy", "modes1", "modes2", "modes3", "points", "set_points", "to_modes_batch", "to_points_batch", "reserve",
       "set_option", "describe", "last_status")


@pytest.fixture(scope="module")
def libpath():
    from fourier_amd import build

    return build.build()


def declared_nufft3d_symbols():
    text = open(os.path.join(ROOT, "include", "fourier.h")).read()
    text = text[: text.index("Header-only C++ RAII wrapper")]
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(fourier_hip_nufft3d_[a-z0-9_]+_(?:float|double))\s*\(", text)))


def test_header_exports_and_binding_name_the_same_nufft3d_symbols(libpath):
    from fourier_amd import _lib

    declared = declared_nufft3d_symbols()
    assert len(declared) == 26
    assert declared == sorted(f"fourier_hip_nufft3d_{op}_{s}" for op in OPS for s in ("float", "double"))
    assert sorted(_lib.NUFFT3D_SYMBOLS) == declared
    out = subprocess.run(["nm", "-D", "--defined-only", libpath], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    assert sorted(s for s in exported if s.startswith("fourier_hip_nufft3d_")) == declared
    assert not set(_lib.NUFFT3D_SYMBOLS) & set(_lib.ALL_SYMBOLS)  # a digit in the name: listed apart, like NUFFT2D_SYMBOLS
    assert not set(_lib.NUFFT3D_SYMBOLS) & set(_lib.NUFFT2D_SYMBOLS)


def test_the_cxx_wrapper_the_cmake_package_and_the_python_layer_name_the_family():
    text = open(os.path.join(ROOT, "include", "fourier.h")).read()
    wrapper = text[text.index("Header-only C++ RAII wrapper"):]
    assert "template <typename T> struct nufft3d;" in wrapper
    for op in OPS:
        assert f"fourier_hip_nufft3d_{op}_##SUFFIX" in wrapper, op
    assert re.search(r"foreach\(FAMILY [^)]*\bnufft3d\b", open(os.path.join(ROOT, "packaging", "CMakeLists.txt")).read())
    import fourier_amd
    from fourier_amd import build

    assert any(group == "nufft3d" and src == "kernels_nufft3d.cpp" for _, src, _, group in build.translation_units())
    for name in ("Nufft3d", "create_nufft3d_f32", "create_nufft3d_f64", "nufft3d1", "nufft3d2"):
        assert hasattr(fourier_amd, name), name
    for method in ("modes", "points", "set_points", "set_points_ptr", "to_modes", "to_modes_ptr", "to_points", "to_points_ptr", "describe",
                   "reserve", "set_option"):
        assert hasattr(fourier_amd.Nufft3d, method), method


def test_every_nufft3d_symbol_resolves_and_the_null_handle_contract_holds_without_a_gpu(libpath):
    from fourier_amd import _lib

    try:  # torch first: one HIP runtime in the process (tests/test_abi.py)
        import torch  # noqa: F401
    except Exception:
        pass
    cdll = _lib.bind(ctypes.CDLL(libpath))
    for sym in _lib.NUFFT3D_SYMBOLS:
        assert getattr(cdll, sym) is not None
    pts = (ctypes.c_double * 3)(0.0, 1.0, 2.0)
    ppts = ctypes.cast(pts, ctypes.c_void_p)
    for s in _lib.SUFFIXES:
        fn = lambda op: getattr(cdll, f"fourier_hip_nufft3d_{op}_{s}")  # noqa: E731
        assert fn("modes1")(None) == 0 and fn("modes2")(None) == 0 and fn("modes3")(None) == 0 and fn("points")(None) == 0
        assert fn("describe")(None) == b""
        assert fn("last_status")(None) == INVALID
        assert fn("reserve")(None, 1) == INVALID
        assert fn("set_option")(None, b"table", 0) == INVALID
        assert fn("set_points")(None, ppts, ppts, ppts, 3, None) == INVALID
        assert fn("to_modes_batch")(None, 16, 64, 1, -1, 0, None) == INVALID
        assert fn("to_points_batch")(None, 16, 64, 1, 1, 0, None) == INVALID
        fn("destroy")(None)
        # refused before a device is looked for: no modes on an axis, an eps that is not a positive finite number, items of modes
        # above 2^30 bytes (one axis alone, a product of two, of three, a product that overflows), a grid item above 2^31 bytes
        for n1, n2, n3, eps in ((0, 4, 4, 1e-6), (4, 0, 4, 1e-6), (4, 4, 0, 1e-6), (8, 8, 8, 0.0), (8, 8, 8, -1.0), (8, 8, 8, float("nan")),
                                (8, 8, 8, float("inf")), (1 << 40, 1, 1, 1e-6), (1, 1 << 40, 1, 1e-6), (1, 1, 1 << 40, 1e-6),
                                (1 << 14, 1 << 14, 1, 1e-6), (1, 1 << 14, 1 << 14, 1e-6), (1 << 9, 1 << 9, 1 << 10, 1e-6),
                                (1 << 22, 1 << 22, 1 << 22, 1e-6), (1 << 33, 1 << 33, 1, 1e-6), (1 << 8, 1 << 9, 1 << 9, 1e-6)):
            assert not fn("create")(n1, n2, n3, eps, -1), (n1, n2, n3, eps)


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
    assert not cdll.fourier_hip_nufft3d_create_float(16, 16, 16, 1e-6, -1)
    with pytest.raises(fourier_amd.FourierError):
        fourier_amd.create_nufft3d_f32((16, 16, 16))
    with pytest.raises(fourier_amd.FourierError):
        fourier_amd.create_nufft3d_f64((30, 4, 9), 1e-12)
    with pytest.raises(ValueError):
        fourier_amd.Nufft3d((0, 3, 3), 1e-6, "f32")
