"""The plan's options in combination and in any order, on the MI355X: tests/option_cases.py through the product library.  The CPU twin
is tests/test_option_emu.py; the two run the same tables and make the same assertions.  Inputs on the device, every output pre-filled
with NaN (in place: with the input) between guard elements.  What the emulation cannot say: the product library refuses the
experiments' options in every state of the two-pass matrix, and a plan that took a run-time kernel ("specialise") keeps it, and its
bits, whatever the Bluestein options are set to afterwards."""
import ctypes
import os
import shutil

import numpy as np
import pytest

import amplitude_cases as cases
import option_cases as options
from test_gpu_amplitude import DeviceApi

pytestmark = pytest.mark.gpu


class FillApi(DeviceApi):
    """DeviceApi whose run() can start from an output that holds `fill` (an in-place call) instead of NaN"""

    def run(self, call, shape, dtype, fill=None):
        count = int(np.prod(shape))
        buf = self.torch.full((count + 2 * cases.GUARD,), cases.SENTINEL, dtype=self.torch.from_numpy(np.empty(0, dtype)).dtype, device="cuda")
        out = buf[cases.GUARD:cases.GUARD + count]
        if fill is None:
            out.fill_(float("nan"))
        else:
            out.copy_(self.put(fill).reshape(-1))
        self.torch.cuda.synchronize()
        call(out.data_ptr())  # on the null stream
        self.torch.cuda.synchronize()
        host = buf.cpu().numpy()
        assert np.all(host[:cases.GUARD] == cases.SENTINEL) and np.all(host[-cases.GUARD:] == cases.SENTINEL), "a guard element was written"
        return host[cases.GUARD:cases.GUARD + count].reshape(shape).copy()


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
    return FillApi(torch, fourier_amd)


@pytest.fixture
def api_experiments(torch, api, monkeypatch):
    """the same sources with the environment switches between plans (fourier_amd/lib/libfourier_experiments.so), for the one route no
    length of test size takes by default: option_cases.GLOBAL_PASS_ENV"""
    from fourier_amd import _lib, build

    if not os.path.exists(build.OUT_EXPERIMENTS):
        pytest.fail("fourier_amd/lib/libfourier_experiments.so is missing: run __graft_entry__.build()")
    monkeypatch.setenv(*options.GLOBAL_PASS_ENV)
    prev = _lib._lib
    _lib._lib = _lib.bind(ctypes.CDLL(build.OUT_EXPERIMENTS))
    yield api
    _lib._lib = prev


@pytest.mark.parametrize("smooth_m", [0, 1, 2])
@pytest.mark.parametrize("name", options.BLU_NAMES)
def test_bluestein_options_in_any_order(api, oracle, name, smooth_m):
    options.check_bluestein(api, oracle, name, smooth_m)


@pytest.mark.parametrize("name", options.BLU_NAMES)
def test_bluestein_states_differ_where_the_rule_says_and_nowhere_else(api, name):
    options.check_bluestein_across_states(api, name)


@pytest.mark.parametrize("which", options.SEQUENCE_NAMES)
def test_a_sequence_gives_what_its_final_values_give(api, which):
    options.check_sequence(api, which)


@pytest.mark.parametrize("real", ["f32", "f64"])
def test_two_pass_options_in_combination(api, real):
    options.check_two_pass(api, real, product=True)


@pytest.mark.parametrize("which", list(options.OTHER_ROUTES))
@pytest.mark.parametrize("real", ["f32", "f64"])
def test_scratch_and_chunk_bytes_change_no_bit_on_every_other_route(request, api, real, which):
    options.check_other_route(request.getfixturevalue("api_experiments") if which == "global passes" else api, which, real)


@pytest.mark.parametrize("real", ["f32", "f64"])
def test_register_stages_there_and_back_between_other_options(api, real):
    options.check_register_stages_interleaved(api, real)


def test_a_specialised_plan_keeps_its_kernel_under_every_bluestein_option(torch, tmp_path):
    """f32 11011 = 7 x 11^2 x 13 is a Bluestein plan by default; "specialise" = 1 compiles its own kernel.  After that every value of
    the five bluestein_* options either returns an error or OK: describe() keeps "specialised" and the output bits stay those right
    after the specialise.  In a child process with a code-object cache of its own: a compiled kernel stays in the process for good, and
    tests/test_gpu_parity.py counts the code objects that ITS compilation of this length leaves in a fresh cache directory."""
    import subprocess
    import sys

    if not (os.path.exists("/opt/rocm/lib/libhiprtc.so") or shutil.which("hipcc")):
        pytest.skip("libhiprtc not installed")
    here = os.path.dirname(os.path.abspath(__file__))
    prog = "import sys; sys.path[:0] = [%r, %r]; import test_gpu_options; test_gpu_options.specialised_child()" % (here, os.path.dirname(here))
    out = subprocess.run([sys.executable, "-c", prog], env=dict(os.environ, FOURIER_HIP_CACHE_DIR=str(tmp_path / "cache")), capture_output=True, text=True, timeout=300)
    print(out.stdout.strip())
    assert out.returncode == 0 and "every call as right after the specialise" in out.stdout, (out.returncode, out.stdout[-2000:], out.stderr[-3000:])


def specialised_child():
    import fourier_amd
    import torch

    api = FillApi(torch, fourier_amd)
    n = 11011
    x = options.inputs(n, "f32", cases.BATCH)
    plan = options.make(api, n, "f32")
    assert plan.describe().startswith("bluestein M="), plan.describe()
    plan.set_option("specialise", 1)
    described = plan.describe()
    assert "specialised" in described and not described.startswith("bluestein"), described
    base = {code: options.call(api, plan, x, code)[0] for code in options.CODES}
    for code in options.CODES:
        assert options.rel_l2(base[code], options.truth(x, code)) <= cases.base_tol(described, "f32"), code
    accepted = refused = 0
    for key, values in zip(options.BLU_KEYS, options.BLU_VALUES):
        for value in values + values[::-1]:
            try:
                plan.set_option(key, value)
                accepted += 1
            except api.fa.FourierError:
                refused += 1
            assert plan.describe() == described, (key, value, plan.describe())
            for code in options.CODES:
                for kind, profiled, in_place in options.KINDS[:2] if code else options.KINDS:
                    assert cases.differing(options.call(api, plan, x, code, profiled, in_place)[0], base[code]) == 0, (key, value, code, kind)
    print(f"options specialised {n} f32: {accepted} settings accepted, {refused} refused; every call as right after the specialise  [{described}]")
