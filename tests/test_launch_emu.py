"""The handles' launch splits WITHOUT a GPU: tests/launch_cases.py on the CPU emulation (tests/emu), whose build reads the development
switches FOURIER_LAUNCH_BYTES and FOURIER_LAUNCH_ITEMS at create as the experiments library does.  The `-m gpu` twin, which runs the
same cases through the experiments library on the MI355X, is tests/test_gpu_launch.py.  Every case asserts that it takes more than one
launch and where the cuts fall, compares with the f64 truth under the handle's own tolerance and with a handle created without the
bound bit for bit; the cases, shapes and bounds are stated there."""
import pytest

import launch_cases as cases

REALS = ["f32", "f64"]


@pytest.fixture(scope="module")
def fa():
    from emu import build_emu
    from fourier_amd import _lib

    prev = _lib._lib
    _lib._lib = build_emu.load()  # route the operator layer to the emulation build
    import fourier_amd

    yield fourier_amd
    _lib._lib = prev
    cases.print_worst()


@pytest.fixture
def api(fa, monkeypatch):
    return cases.HostApi(fa, monkeypatch)


def test_a_launch_bound_is_never_above_the_kernels_range_and_zero_is_no_bound(fa, monkeypatch):
    """launch_bound (handle_common.h): a switch above the constant, or 0, leaves the constant -- the call runs in one launch and gives the
    unbounded handle's bits"""
    import numpy as np

    rng = np.random.default_rng(1)
    x = cases.randn(rng, (3, 64), np.float32)
    got = []
    for value in (None, "0", str(1 << 40)):
        if value is not None:
            monkeypatch.setenv(cases.BYTES, value)
            monkeypatch.setenv(cases.ITEMS, value)
        plan = fa.RealFft(64, "f32")
        out = np.empty((3, 33), np.complex64)
        plan.forward_batch_ptr(x.ctypes.data, out.ctypes.data, 3)
        got.append(out)
    assert cases.same_bits(got[0], got[1]) and cases.same_bits(got[0], got[2])


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
    cases.xcorr_one_launch(api, real, {"FOURIER_XCORR_SPILLING": 1})


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
