"""A non-finite value stays in its own row, frame and sample on the MI355X: tests/isolation_cases.py through the product library.  The
CPU twin is tests/test_isolation_emu.py; the two run the same cases and make the same assertions, all of them bit for bit against the
clean run of the same handle: (A) a unit of any input filled with NaN reaches the output units the f64 truth says it reaches and no
other, (B) one +Inf sample, or frame of an inverse, reaches the frames or samples the framing gives, (C) the inputs between two bands
of NaN in one allocation give the clean result, (D) so do the clean inputs after the poisoned calls on the same handle.  What the
emulation cannot say: the product's route tables are not the emulator's, the hardware's buffer descriptors decide what a load beyond
a row returns, and the packed-f32 kernels exist only here.  tests/test_gpu_parity.py's
test_a_non_finite_transform_does_not_reach_its_neighbours keeps the core plans' batches of 19 to 70 (a lane per transform, several
rows per workgroup), which the table's batch of 3 does not reach."""
import pytest

import amplitude_cases as cases
import isolation_cases as isolation
from test_gpu_amplitude import DeviceApi

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch():
    import torch

    if not torch.cuda.is_available():
        pytest.fail("these tests need a GPU: the product path has no CPU fallback")
    return torch


@pytest.fixture(scope="module")
def api(torch):
    import fourier_amd
    from fourier_amd import _lib

    _lib.lib()
    assert "fourier_amd/lib/libfourier.so" in open("/proc/self/maps").read()
    return DeviceApi(torch, fourier_amd)  # Banded's slice of a device tensor keeps the bands in the data's allocation


def test_every_case_has_exactly_one_unit_view():
    for case in cases.CASES:
        isolation.view_of(case)


@pytest.mark.parametrize("name", cases.NAMES)
@pytest.mark.parametrize("real", ["f32", "f64"])
def test_a_non_finite_value_stays_in_its_units(api, real, name):
    isolation.check_isolation(api, cases.BY_NAME[name], real)
