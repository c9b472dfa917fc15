"""The amplitude range on the MI355X: tests/amplitude_cases.py through the product library.  The CPU twin is
tests/test_amplitude_emu.py; the two run the same cases and make the same assertions: (a) f(2^k x) bit-equal to 2^(k d) f(x) -- and,
for the cross-correlation and GCC-PHAT, x 2^k against y 2^-k with no bit changed --, (b) the families' tolerances against the f64
truth at the extreme k (the cepstrum also against its own k = 0 result at every k), (c) integer-valued samples in f32 and the
two-tone coherence, (d) the range edge of the magnitude paths, of GCC-PHAT and of the cepstrum.  What the emulation cannot say is
whether the device's arithmetic -- contracted multiply-adds, its division and square root, its logf / expf, its treatment of
subnormals -- keeps (a); the k of the cases keep every value normal."""
import numpy as np
import pytest

import amplitude_cases as cases

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch():
    import torch

    if not torch.cuda.is_available():
        pytest.fail("these tests need a GPU: the product path has no CPU fallback")
    return torch


class DeviceApi:
    """tests/amplitude_cases.py's adapter for the product library: inputs on the device, every output between guard elements in one
    allocation, results back as numpy arrays"""
    device = 0

    def __init__(self, torch, fa):
        self.torch, self.fa = torch, fa

    def put(self, a):
        return self.torch.from_numpy(np.ascontiguousarray(a)).cuda()

    def ptr(self, b):
        return b.data_ptr()

    def run(self, call, shape, dtype):
        count = int(np.prod(shape))
        buf = self.torch.full((count + 2 * cases.GUARD,), cases.SENTINEL, dtype=self.torch.from_numpy(np.empty(0, dtype)).dtype, device="cuda")
        out = buf[cases.GUARD:cases.GUARD + count]
        out.fill_(float("nan"))
        self.torch.cuda.synchronize()
        call(out.data_ptr())  # on the null stream
        self.torch.cuda.synchronize()
        host = buf.cpu().numpy()
        assert np.all(host[:cases.GUARD] == cases.SENTINEL) and np.all(host[-cases.GUARD:] == cases.SENTINEL), "a guard element was written"
        return host[cases.GUARD:cases.GUARD + count].reshape(shape).copy()


@pytest.fixture(scope="module")
def api(torch):
    import fourier_amd
    from fourier_amd import _lib

    _lib.lib()
    assert "fourier_amd/lib/libfourier.so" in open("/proc/self/maps").read()
    return DeviceApi(torch, fourier_amd)


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
