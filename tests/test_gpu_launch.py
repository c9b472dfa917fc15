"""The handles' launch splits on the MI355X: tests/launch_cases.py through fourier_amd/lib/libfourier_experiments.so, which is built from
the product's objects and reads the development switches FOURIER_LAUNCH_BYTES and FOURIER_LAUNCH_ITEMS at create (launch_bound,
handle_common.h).  The product library never reads them, so there every one of these loops takes a single turn at test shapes; here
every split walks several launches at batches of 3 to 7.  The CPU twin, which runs the same cases on the emulation, is
tests/test_launch_emu.py.  Every case asserts where the cuts fall, compares with the f64 truth under the handle's own tolerance and
with a handle created without the bound bit for bit, between guard elements; the cases, shapes and bounds are stated in
tests/launch_cases.py."""
import ctypes
import os

import numpy as np
import pytest

import launch_cases as cases

pytestmark = pytest.mark.gpu

REALS = ["f32", "f64"]
GUARD = 64
SENTINEL = 77.0


@pytest.fixture(scope="module")
def torch():
    import torch

    if not torch.cuda.is_available():
        pytest.fail("these tests need a GPU: the product path has no CPU fallback")
    return torch


@pytest.fixture(scope="module")
def fa(torch):
    import fourier_amd
    from fourier_amd import _lib

    _lib.lib()
    assert "fourier_amd/lib/libfourier.so" in open("/proc/self/maps").read()
    yield fourier_amd
    cases.print_worst()


@pytest.fixture
def fx(torch, fa):
    """fourier_amd bound to the experiments library for one test; a handle keeps the library it was created from"""
    from fourier_amd import _lib, build

    if not os.path.exists(build.OUT_EXPERIMENTS):
        pytest.fail("fourier_amd/lib/libfourier_experiments.so is missing: run __graft_entry__.build()")
    prev = _lib._lib
    _lib._lib = _lib.bind(ctypes.CDLL(build.OUT_EXPERIMENTS))
    yield fa
    _lib._lib = prev


class DeviceApi:
    """tests/launch_cases.py's adapter for the experiments library: inputs on the device, every output between GUARD sentinel elements in
    one allocation, prefilled with NaN, results back as numpy arrays"""

    def __init__(self, torch, fx, monkeypatch):
        self.torch, self.fa, self.monkeypatch = torch, fx, monkeypatch

    def create(self, make, **env):
        """make(fa) with the development switches `env` set: they are read at create only"""
        for k, v in env.items():
            self.monkeypatch.setenv(k, str(v))
        try:
            return make(self.fa)
        finally:
            for k in env:
                self.monkeypatch.delenv(k)

    def put(self, a):
        return self.torch.from_numpy(a).cuda()

    def ptr(self, buf):
        return buf.data_ptr()

    def get(self, buf):
        return buf.cpu().numpy()

    def run(self, call, shape, dtype):
        torch = self.torch
        dt = {np.dtype(np.float32): torch.float32, np.dtype(np.float64): torch.float64, np.dtype(np.complex64): torch.complex64,
              np.dtype(np.complex128): torch.complex128}[np.dtype(dtype)]
        count = int(np.prod(shape))
        buf = torch.full((count + 2 * GUARD,), SENTINEL, dtype=dt, device="cuda")
        out = buf[GUARD:GUARD + count]
        out.fill_(float("nan"))
        call(out.data_ptr())  # the entry points enqueue on the null stream, which the copies below wait for
        host = buf.cpu().numpy()
        assert np.all(host[:GUARD] == SENTINEL) and np.all(host[-GUARD:] == SENTINEL), "a guard element was written"
        return host[GUARD:GUARD + count].reshape(shape).copy()


@pytest.fixture
def api(torch, fx, monkeypatch):
    return DeviceApi(torch, fx, monkeypatch)


def test_the_product_library_does_not_read_the_launch_switches(torch, fa, monkeypatch):
    """libfourier.so under both switches: the bits of a handle created without them (dev_env returns nothing there)"""
    g = torch.Generator(device="cuda").manual_seed(1)
    x = torch.randn(7, 250, dtype=torch.float32, device="cuda", generator=g)
    plain = fa.Hilbert(250, "f32")
    monkeypatch.setenv(cases.BYTES, "8")
    monkeypatch.setenv(cases.ITEMS, "1")
    switched = fa.Hilbert(250, "f32")
    assert switched._L._name.endswith("libfourier.so") and switched.describe() == plain.describe()
    assert torch.equal(torch.view_as_real(switched.analytic(x)), torch.view_as_real(plain.analytic(x)))


@pytest.mark.parametrize("n", [64, 250])
@pytest.mark.parametrize("real", REALS)
def test_real_plan_sweep(api, real, n):
    cases.real_sweep(api, real, n)


@pytest.mark.parametrize("n", [64, 250])
@pytest.mark.parametrize("real", REALS)
def test_r2r_plan_sweep(api, real, n):
    cases.r2r_sweep(api, real, n)


@pytest.mark.parametrize("n", [64, 250, 63])
@pytest.mark.parametrize("real", REALS)
def test_hilbert_sweep(api, real, n):
    cases.hilbert_sweep(api, real, n)


@pytest.mark.parametrize("real", REALS)
def test_hilbert_one_launch_rows(api, real):
    cases.hilbert_one_launch(api, real)


@pytest.mark.parametrize("real_input", [False, True], ids=["complex", "real"])
@pytest.mark.parametrize("shape", cases.CZT_SHAPES, ids=lambda s: f"{s[0]}-{s[1]}")
@pytest.mark.parametrize("real", REALS)
def test_czt_sweep_and_multiply(api, real, shape, real_input):
    cases.czt_sweep(api, real, shape[0], shape[1], real_input)


@pytest.mark.parametrize("real", REALS)
def test_czt_one_launch_rows(api, real):
    cases.czt_one_launch(api, real)


@pytest.mark.parametrize("shape", cases.RESAMPLE_SHAPES, ids=lambda s: f"{s[0]}-{s[1]}-{'complex' if s[2] else 'real'}-fusion{s[3]}")
@pytest.mark.parametrize("real", REALS)
def test_resample_sweep(api, real, shape):
    cases.resample_sweep(api, real, *shape)


@pytest.mark.parametrize("shape", cases.CONV_SHAPES, ids=lambda s: f"{s[0]}-{'real' if s[1] else 'complex'}-fusion{s[2]}")
@pytest.mark.parametrize("real", REALS)
def test_conv_sweep_and_the_filter_a_launch_starts_on(api, real, shape):
    cases.conv_sweep(api, real, *shape)


@pytest.mark.parametrize("real_data", [True, False], ids=["real", "complex"])
@pytest.mark.parametrize("real", REALS)
def test_xcorr_sweep(api, real, real_data):
    cases.xcorr_sweep(api, real, 40, 64, real_data)
    cases.xcorr_sweep(api, real, 63, 63, real_data)


@pytest.mark.parametrize("real", REALS)
def test_xcorr_one_launch_rows(api, real):
    """f64 has a one-launch kernel in every build; f32's is the spilling one the experiments library selects on request
    (tests/test_gpu_xcorr.py)"""
    cases.xcorr_one_launch(api, real, {"FOURIER_XCORR_SPILLING": 1} if real == "f32" else {})


@pytest.mark.parametrize("overlap_save", [1, 0], ids=["overlap-save", "padded"])
@pytest.mark.parametrize("real_data", [True, False], ids=["real", "complex"])
@pytest.mark.parametrize("real", REALS)
def test_lconv_apply_and_copy_rows(api, real, real_data, overlap_save):
    cases.lconv_split(api, real, real_data, overlap_save)


@pytest.mark.parametrize("frames", [None, 5], ids=["ragged", "one-frame"])
@pytest.mark.parametrize("real", REALS)
def test_fused_frame_routes(api, real, frames):
    cases.stft_frames(api, real, frames)
    cases.spectrogram_frames(api, real, frames)
    cases.bandspec_frames(api, real, frames)
    cases.mdct_frames(api, real, frames)
    for real_input in (True, False):
        cases.pfb_frames(api, real, real_input, frames)


@pytest.mark.parametrize("real", REALS)
def test_composed_frame_routes(api, real):
    cases.composed_frames(api, real)


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "composed"])
@pytest.mark.parametrize("real", REALS)
def test_welch_and_csd_row_groups(api, real, fused):
    cases.welch_groups(api, real, fused)
    cases.csd_groups(api, real, fused)


@pytest.mark.parametrize("hop", [12, 20])
@pytest.mark.parametrize("real_output", [True, False], ids=["real", "complex"])
@pytest.mark.parametrize("real", REALS)
def test_ipfb_gather(api, real, real_output, hop):
    cases.ipfb_gather(api, real, real_output, hop)
