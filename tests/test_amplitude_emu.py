"""The amplitude range WITHOUT a GPU: tests/amplitude_cases.py on the CPU emulation (tests/emu) -- the same kernel sources in CPU
arithmetic, driven through the same C ABI / Python layer as the product.  The `-m gpu` twin is tests/test_gpu_amplitude.py; the two run
the same cases and make the same assertions: (a) f(2^k x) bit-equal to 2^(k d) f(x) -- and, for the cross-correlation and GCC-PHAT,
x 2^k against y 2^-k with no bit changed --, (b) the families' tolerances against the f64 truth at the extreme k (the cepstrum also
against its own k = 0 result at every k), (c) integer-valued samples in f32 and the two-tone coherence, (d) the range edge of the
magnitude paths, of GCC-PHAT and of the cepstrum."""
import pytest

import amplitude_cases as cases


@pytest.fixture(scope="module")
def api():
    from emu import build_emu
    from fourier_amd import _lib

    prev = _lib._lib
    _lib._lib = build_emu.load()  # route the operator layer to the emulation build
    import fourier_amd

    yield cases.HostApi(fourier_amd)
    _lib._lib = prev


@pytest.mark.parametrize("name", cases.NAMES)
@pytest.mark.parametrize("real", ["f32", "f64"])
def test_scaling_is_exact_and_the_truth_holds_at_amplitude(api, real, name):
    cases.check_scaling(api, cases.BY_NAME[name], real)


@pytest.mark.parametrize("name", cases.INTEGER_NAMES)
def test_integer_valued_samples(api, name):
    cases.check_integers(api, cases.BY_NAME[name])


def test_two_full_scale_tones_have_a_finite_coherence(api):
    cases.two_tone(api)


@pytest.mark.parametrize("name", cases.EDGE_NAMES)
@pytest.mark.parametrize("real", ["f32", "f64"])
def test_magnitude_range_edge(api, real, name):
    cases.check_edge(api, cases.BY_NAME[name], real)
