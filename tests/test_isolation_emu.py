"""A non-finite value stays in its own row, frame and sample WITHOUT a GPU: tests/isolation_cases.py on the CPU emulation (tests/emu) --
the same kernel sources in CPU arithmetic, driven through the same C ABI / Python layer as the product.  The `-m gpu` twin is
tests/test_gpu_isolation.py; the two run the same cases and make the same assertions, all of them bit for bit against the clean run of
the same handle: (A) a unit of any input filled with NaN reaches the output units the f64 truth says it reaches and no other, (B) one
+Inf sample, or frame of an inverse, reaches the frames or samples the framing gives, (C) the inputs between two bands of NaN in one
allocation give the clean result, (D) so do the clean inputs after the poisoned calls on the same handle."""
import pytest

import amplitude_cases as cases
import isolation_cases as isolation


@pytest.fixture(scope="module")
def api():
    from emu import build_emu
    from fourier_amd import _lib

    prev = _lib._lib
    _lib._lib = build_emu.load()  # route the operator layer to the emulation build
    import fourier_amd

    yield cases.HostApi(fourier_amd)
    _lib._lib = prev


def test_every_case_has_exactly_one_unit_view():
    for case in cases.CASES:
        isolation.view_of(case)


@pytest.mark.parametrize("name", cases.NAMES)
@pytest.mark.parametrize("real", ["f32", "f64"])
def test_a_non_finite_value_stays_in_its_units(api, real, name):
    isolation.check_isolation(api, cases.BY_NAME[name], real)
