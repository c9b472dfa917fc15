"""Host-side mirror of the reference's operator interface for the FFT path.

Same names, argument meaning and error behaviour as the reference:
  * `Transform`                  -- fourier-algorithms/src/fft.rs:4-37
  * `Fft` (size / transform_in_place / transform / fft / ifft ...) -- fft.rs:40-82
  * `create_fft_f32`, `create_fft_f64` -- fourier/src/lib.rs:31-60
plus the batched, device-resident entry point the GPU path is measured on (the reference has no
batch API: fft.rs:48-61 takes one slice per call).

Buffers: numpy complex64/complex128 arrays go through the legacy host ABI (H2D + D2H inside the
library; arrays holding several transforms are streamed through the device in chunks); torch CUDA
tensors go through the device-resident batched ABI on the current stream.
All compute happens in libfourier.so (HIP); there is no CPU fallback.
"""
import enum

import numpy as np

from . import _lib


class Transform(enum.IntEnum):
    """fourier-algorithms/src/fft.rs:4-16; integer values = the C codes (fourier-ffi/src/lib.rs:3-12)."""

    Fft = 0
    Ifft = 1
    UnscaledIfft = 2
    SqrtScaledFft = 3
    SqrtScaledIfft = 4

    def is_forward(self):  # fft.rs:20-25
        return self in (Transform.Fft, Transform.SqrtScaledFft)

    def inverse(self):  # fft.rs:28-36
        return {Transform.Fft: Transform.Ifft, Transform.Ifft: Transform.Fft,
                Transform.SqrtScaledFft: Transform.SqrtScaledIfft,
                Transform.SqrtScaledIfft: Transform.SqrtScaledFft}.get(self)


class FourierError(RuntimeError):
    pass


def _is_torch(x):
    return type(x).__module__.startswith("torch")


class Fft:
    """The `Fft` trait (fft.rs:40-82) over a libfourier.so plan handle."""

    def __init__(self, size, real, device=-1):
        self._suffix = {"f32": "float", "f64": "double"}[real]
        self.real = real
        self.np_dtype = np.dtype(np.complex64 if real == "f32" else np.complex128)
        self._L = _lib.lib()
        self._h = getattr(self._L, f"fourier_hip_create_{self._suffix}")(int(size), int(device))
        if not self._h:
            # the reference's create panics -> NULL through the FFI (fourier-ffi/src/lib.rs:18-19)
            raise FourierError(f"cannot create FFT plan of size {size}")
        self._n = int(size)
        self.device = int(getattr(self._L, f"fourier_hip_device_{self._suffix}")(self._h))  # device=-1 binds the current one

    # -- trait surface ---------------------------------------------------------------------
    def size(self):
        return self._n

    def transform_in_place(self, input, transform):
        """fft.rs:48: in-place transform of exactly `size` elements (or batch*size, see below)."""
        self._dispatch(input, input, transform)

    def transform(self, input, output, transform):
        """fft.rs:51-61: out-of-place; asserts both lengths equal size()."""
        self._dispatch(input, output, transform)

    def fft_in_place(self, input):  # fft.rs:64-66
        self.transform_in_place(input, Transform.Fft)

    def ifft_in_place(self, input):  # fft.rs:69-71
        self.transform_in_place(input, Transform.Ifft)

    def fft(self, input, output):  # fft.rs:74-76
        self.transform(input, output, Transform.Fft)

    def ifft(self, input, output):  # fft.rs:79-81
        self.transform(input, output, Transform.Ifft)

    # -- batched device-resident extension -------------------------------------------------
    def transform_batch_ptr(self, d_in, d_out, batch, transform, stream=0):
        """Raw-pointer form: `batch` contiguous transforms on device memory, enqueued on `stream`."""
        st = getattr(self._L, f"fourier_hip_transform_batch_{self._suffix}")(
            self._h, d_in, d_out, int(batch), int(transform), stream)
        if st != 0:
            raise FourierError(self._L.fourier_hip_status_string(st).decode())

    def transform_batch_host(self, input, output, transform):
        """`batch` contiguous transforms in host (numpy) memory, streamed through the device in chunks with
        copies and kernels overlapped; synchronous.  input may be output (in place)."""
        for a in (input, output):
            if not (isinstance(a, np.ndarray) and a.dtype == self.np_dtype and a.flags.c_contiguous):
                raise TypeError(f"expected C-contiguous numpy {self.np_dtype} arrays")
        if input.size != output.size or input.size % self._n != 0:
            raise ValueError(f"buffers of {input.size}/{output.size} elements are not the same whole number of transforms")
        st = getattr(self._L, f"fourier_hip_transform_batch_host_{self._suffix}")(
            self._h, input.ctypes.data, output.ctypes.data, input.size // self._n, int(transform))
        if st != 0:
            raise FourierError(self._L.fourier_hip_status_string(st).decode())

    def synchronize(self, stream=0):
        """Blocks until everything queued on `stream` (a HIP stream handle, 0 = the NULL stream) of the plan's device has
        finished: the wait that follows a stream-ordered transform_batch_ptr when no other runtime owns the stream."""
        st = getattr(self._L, f"fourier_hip_synchronize_{self._suffix}")(self._h, stream)
        if st != 0:
            raise FourierError(self._L.fourier_hip_status_string(st).decode())

    def reserve(self, batch, in_place=False):
        """Pre-size the plan-owned device buffers so that later batched calls of up to `batch` transforms never
        allocate (hipMalloc synchronises the device; needed before HIP-graph capture)."""
        st = getattr(self._L, f"fourier_hip_reserve_{self._suffix}")(self._h, int(batch), int(bool(in_place)))
        if st != 0:
            raise FourierError(self._L.fourier_hip_status_string(st).decode())

    def profile_batch_ptr(self, d_in, d_out, batch, transform, stream=0, nslots=16):
        """One batched transform with a HIP event pair around every kernel launch.
        Returns [(slot_name, total_ms, launches), ...] in launch order."""
        import ctypes

        ms = (ctypes.c_float * nslots)()
        cnt = (ctypes.c_int * nslots)()
        st = getattr(self._L, f"fourier_hip_profile_{self._suffix}")(
            self._h, d_in, d_out, int(batch), int(transform), stream, nslots, ms, cnt)
        if st != 0:
            raise FourierError(self._L.fourier_hip_status_string(st).decode())
        names = getattr(self._L, f"fourier_hip_slot_names_{self._suffix}")(self._h).decode().split(",")
        return [(nm, float(ms[i]), int(cnt[i])) for i, nm in enumerate(names) if i < nslots]

    def set_option(self, key, value):
        st = getattr(self._L, f"fourier_hip_set_option_{self._suffix}")(self._h, key.encode(), int(value))
        if st != 0:
            raise FourierError(f"bad option {key}={value}")

    def describe(self):
        return getattr(self._L, f"fourier_hip_describe_{self._suffix}")(self._h).decode()

    def model_bytes(self):
        return getattr(self._L, f"fourier_hip_model_bytes_{self._suffix}")(self._h)

    # -- transforms along a strided axis (extension) -----------------------------------------
    def transform_axis_ptr(self, d_in, d_out, outer, inner, transform, stream=0):
        """Raw-pointer form: the middle axis of an [outer][size][inner] complex array on device memory, enqueued on `stream`."""
        st = getattr(self._L, f"fourier_hip_transform_axis_{self._suffix}")(
            self._h, d_in, d_out, int(outer), int(inner), int(transform), stream)
        if st != 0:
            raise FourierError(self._L.fourier_hip_status_string(st).decode())

    def reserve_axis(self, outer, inner):
        """Pre-size the plan-owned buffers so that later axis calls of at most outer x inner never allocate."""
        st = getattr(self._L, f"fourier_hip_reserve_axis_{self._suffix}")(self._h, int(outer), int(inner))
        if st != 0:
            raise FourierError(self._L.fourier_hip_status_string(st).decode())

    def describe_axis(self, inner):
        """The route an axis call with this `inner` takes (include/fourier.h)."""
        return getattr(self._L, f"fourier_hip_describe_axis_{self._suffix}")(self._h, int(inner)).decode()

    def transform_axis(self, input, output, transform, dim):
        """Transform contiguous CUDA complex tensors along dimension `dim` (shape[dim] == size()), on the current stream.
        input may be output (in place); any other overlap is refused."""
        import torch

        want = torch.complex64 if self.real == "f32" else torch.complex128
        for t in (input, output):
            if not (_is_torch(t) and t.is_cuda and t.dtype == want and t.is_contiguous()):
                raise TypeError(f"expected contiguous CUDA {want} tensors")
            if t.device.index != self.device:
                raise ValueError(f"tensor on cuda:{t.device.index}, plan on cuda:{self.device}")
        if input.shape != output.shape:
            raise ValueError(f"shapes {tuple(input.shape)} and {tuple(output.shape)} differ")
        nd = input.dim()
        if not -nd <= dim < nd:
            raise ValueError(f"dim {dim} out of range for {nd} dimensions")
        dim %= nd
        if input.shape[dim] != self._n:
            raise ValueError(f"dimension {dim} has {input.shape[dim]} elements, plan size is {self._n}")
        a0, b0 = input.data_ptr(), output.data_ptr()
        nbytes = input.numel() * input.element_size()
        if a0 != b0 and a0 < b0 + nbytes and b0 < a0 + nbytes:
            raise ValueError("input and output overlap partially")
        outer = 1
        for d in input.shape[:dim]:
            outer *= d
        inner = 1
        for d in input.shape[dim + 1:]:
            inner *= d
        if outer * inner == 0:
            return
        stream = torch.cuda.current_stream(input.device).cuda_stream
        self.transform_axis_ptr(a0, b0, outer, inner, int(transform), stream)

    # -- plumbing --------------------------------------------------------------------------
    def _dispatch(self, input, output, transform):
        code = int(transform)
        if _is_torch(input) or _is_torch(output):
            import torch

            want = torch.complex64 if self.real == "f32" else torch.complex128
            for t in (input, output):
                if not (_is_torch(t) and t.is_cuda and t.dtype == want and t.is_contiguous()):
                    raise TypeError(f"expected contiguous CUDA {want} tensors")
            # the reference asserts input.len() == output.len() == size (fft.rs:57-58); the batched
            # extension accepts any whole number of transforms
            if input.numel() != output.numel() or input.numel() % self._n != 0 or input.numel() == 0:
                raise ValueError(f"buffer of {input.numel()} elements is not a multiple of size {self._n}")
            # the plan's tables, scratch and kernels live on ONE device (fixed at creation)
            for t in (input, output):
                if t.device.index != self.device:
                    raise ValueError(f"tensor on cuda:{t.device.index}, plan on cuda:{self.device}")
            # same buffer = in place; anything else must not overlap (include/fourier.h)
            a0, b0 = input.data_ptr(), output.data_ptr()
            nbytes = input.numel() * input.element_size()
            if a0 != b0 and a0 < b0 + nbytes and b0 < a0 + nbytes:
                raise ValueError("input and output overlap partially")
            stream = torch.cuda.current_stream(input.device).cuda_stream
            self.transform_batch_ptr(input.data_ptr(), output.data_ptr(), input.numel() // self._n, code, stream)
            return
        for a in (input, output):
            if not (isinstance(a, np.ndarray) and a.dtype == self.np_dtype and a.flags.c_contiguous):
                raise TypeError(f"expected C-contiguous numpy {self.np_dtype} arrays")
        if not output.flags.writeable:
            raise ValueError("output is read-only")
        if input.size == output.size and input.size > self._n and input.size % self._n == 0:
            # several whole transforms in host memory: streamed through the device (extension)
            self.transform_batch_host(input, output, transform)
            return
        if input.size != self._n or output.size != self._n:
            raise ValueError(f"buffer length {input.size}/{output.size} != size {self._n}")  # fft.rs:57-58
        if input is output or input.ctypes.data == output.ctypes.data:
            getattr(self._L, f"fourier_transform_in_place_{self._suffix}")(self._h, output.ctypes.data, code)
        else:
            getattr(self._L, f"fourier_transform_{self._suffix}")(self._h, input.ctypes.data, output.ctypes.data, code)
        st = getattr(self._L, f"fourier_hip_last_status_{self._suffix}")(self._h)
        if st != 0:
            raise FourierError(self._L.fourier_hip_status_string(st).decode())

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            try:
                getattr(self._L, f"fourier_destroy_{self._suffix}")(h)
            except Exception:
                pass


class RealFft:
    """Batched real-input transforms (include/fourier.h, fourier_hip_real_*): N reals per row <-> N//2+1 complex per row, numpy's
    rfft / irfft layout, on device memory.  Forward codes Fft / SqrtScaledFft, inverse codes Ifft / UnscaledIfft / SqrtScaledIfft."""

    def __init__(self, size, real, device=-1):
        self._suffix = {"f32": "float", "f64": "double"}[real]
        self.real = real
        self._L = _lib.lib()
        self._h = getattr(self._L, f"fourier_hip_real_create_{self._suffix}")(int(size), int(device))
        if not self._h:
            raise FourierError(f"cannot create real FFT plan of size {size}")
        self._n = int(size)

    def size(self):
        return self._n

    def describe(self):
        return getattr(self._L, f"fourier_hip_real_describe_{self._suffix}")(self._h).decode()

    def _check(self, st):
        if st != 0:
            raise FourierError(self._L.fourier_hip_status_string(st).decode())

    def forward_batch_ptr(self, d_in, d_out, batch, transform=Transform.Fft, stream=0):
        """`batch` rows of N reals at d_in -> `batch` rows of N//2+1 complex at d_out, enqueued on `stream`."""
        self._check(getattr(self._L, f"fourier_hip_real_forward_batch_{self._suffix}")(
            self._h, d_in, d_out, int(batch), int(transform), stream))

    def inverse_batch_ptr(self, d_in, d_out, batch, transform=Transform.Ifft, stream=0):
        """`batch` rows of N//2+1 complex at d_in -> `batch` rows of N reals at d_out (d_in is not modified)."""
        self._check(getattr(self._L, f"fourier_hip_real_inverse_batch_{self._suffix}")(
            self._h, d_in, d_out, int(batch), int(transform), stream))

    def reserve(self, batch):
        """Pre-size the plan-owned buffers: later calls of at most `batch` rows never allocate."""
        self._check(getattr(self._L, f"fourier_hip_real_reserve_{self._suffix}")(self._h, int(batch)))

    def _tensor(self, x, dtype, last):
        import torch

        if not (_is_torch(x) and x.is_cuda and x.dtype == dtype and x.is_contiguous()):
            raise TypeError(f"expected a contiguous CUDA {dtype} tensor")
        if x.dim() == 0 or x.shape[-1] != last:
            raise ValueError(f"last dimension must be {last}, got {tuple(x.shape)}")
        return torch.cuda.current_stream(x.device).cuda_stream

    def rfft(self, x, transform=Transform.Fft):
        """Contiguous (..., N) float32 / float64 CUDA tensor -> new (..., N//2+1) complex tensor, on the current stream."""
        import torch

        real_dt, cpx_dt = (torch.float32, torch.complex64) if self.real == "f32" else (torch.float64, torch.complex128)
        stream = self._tensor(x, real_dt, self._n)
        out = torch.empty(x.shape[:-1] + (self._n // 2 + 1,), dtype=cpx_dt, device=x.device)
        batch = x.numel() // self._n
        if batch:
            self.forward_batch_ptr(x.data_ptr(), out.data_ptr(), batch, transform, stream)
        return out

    def irfft(self, X, transform=Transform.Ifft):
        """Contiguous (..., N//2+1) complex CUDA tensor -> new (..., N) real tensor, on the current stream; X is not modified."""
        import torch

        real_dt, cpx_dt = (torch.float32, torch.complex64) if self.real == "f32" else (torch.float64, torch.complex128)
        stream = self._tensor(X, cpx_dt, self._n // 2 + 1)
        out = torch.empty(X.shape[:-1] + (self._n,), dtype=real_dt, device=X.device)
        batch = X.numel() // (self._n // 2 + 1)
        if batch:
            self.inverse_batch_ptr(X.data_ptr(), out.data_ptr(), batch, transform, stream)
        return out

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            try:
                getattr(self._L, f"fourier_hip_real_destroy_{self._suffix}")(h)
            except Exception:
                pass


def create_rfft_f32(size, device=-1):
    return RealFft(size, "f32", device)


def create_rfft_f64(size, device=-1):
    return RealFft(size, "f64", device)


class FftConv:
    """Batched circular convolution / correlation with a prepared filter bank (include/fourier.h, fourier_hip_conv_*) on device
    memory: rows of N complex values (real_data=False) or N reals (real_data=True) in, rows of the same shape out, row b with filter
    b mod F.  The filters are given in the time domain (set_filters) and transformed once."""

    def __init__(self, size, real, real_data=False, device=-1):
        self._suffix = {"f32": "float", "f64": "double"}[real]
        self.real = real
        self.real_data = bool(real_data)
        self._L = _lib.lib()
        self._h = getattr(self._L, f"fourier_hip_conv_create_{self._suffix}")(int(size), int(self.real_data), int(device))
        if not self._h:
            raise FourierError(f"cannot create convolution plan of size {size}")
        self._n = int(size)

    def size(self):
        return self._n

    def filters(self):
        return int(getattr(self._L, f"fourier_hip_conv_filters_{self._suffix}")(self._h))

    def describe(self):
        return getattr(self._L, f"fourier_hip_conv_describe_{self._suffix}")(self._h).decode()

    def _check(self, st):
        if st != 0:
            raise FourierError(self._L.fourier_hip_status_string(st).decode())

    def set_option(self, key, value):
        """"fusion": 1 (default) / 0 = the composed route (forward transform, product sweep, inverse transform)."""
        self._check(getattr(self._L, f"fourier_hip_conv_set_option_{self._suffix}")(self._h, key.encode(), int(value)))

    def reserve(self, batch):
        """Pre-size the plan-owned buffers: later apply calls of at most `batch` rows never allocate."""
        self._check(getattr(self._L, f"fourier_hip_conv_reserve_{self._suffix}")(self._h, int(batch)))

    def set_filters_ptr(self, d_taps, taps, filters=1, correlate=False, stream=0):
        """`filters` rows of `taps` values of the handle's kind at d_taps -> the bank, enqueued on `stream`."""
        self._check(getattr(self._L, f"fourier_hip_conv_set_filters_{self._suffix}")(
            self._h, d_taps, int(taps), int(filters), int(bool(correlate)), stream))

    def apply_ptr(self, d_in, d_out, batch, stream=0):
        """`batch` rows of N values at d_in -> `batch` rows at d_out (d_out may be d_in), enqueued on `stream`."""
        self._check(getattr(self._L, f"fourier_hip_conv_apply_{self._suffix}")(self._h, d_in, d_out, int(batch), stream))

    def _dtype(self):
        import torch

        if self.real_data:
            return torch.float32 if self.real == "f32" else torch.float64
        return torch.complex64 if self.real == "f32" else torch.complex128

    def set_filters(self, taps, correlate=False):
        """Contiguous CUDA tensor of shape (taps,) or (F, taps), of the handle's dtype, 1 <= taps <= N; on the current stream."""
        import torch

        dtype = self._dtype()
        if not (_is_torch(taps) and taps.is_cuda and taps.dtype == dtype and taps.is_contiguous()):
            raise TypeError(f"expected a contiguous CUDA {dtype} tensor")
        if taps.dim() not in (1, 2) or taps.numel() == 0 or taps.shape[-1] > self._n:
            raise ValueError(f"taps must have shape (taps,) or (F, taps) with 1 <= taps <= {self._n}, got {tuple(taps.shape)}")
        stream = torch.cuda.current_stream(taps.device).cuda_stream
        self.set_filters_ptr(taps.data_ptr(), taps.shape[-1], taps.numel() // taps.shape[-1], correlate, stream)

    def apply(self, x, out=None):
        """Contiguous (..., N) CUDA tensor of the handle's dtype -> a new tensor of the same shape, or `out` (which may be `x`), on
        the current stream.  Row b of the flattened leading dimensions uses filter b mod F."""
        import torch

        dtype = self._dtype()
        if not (_is_torch(x) and x.is_cuda and x.dtype == dtype and x.is_contiguous()):
            raise TypeError(f"expected a contiguous CUDA {dtype} tensor")
        if x.dim() == 0 or x.shape[-1] != self._n:
            raise ValueError(f"last dimension must be {self._n}, got {tuple(x.shape)}")
        if out is None:
            out = torch.empty_like(x)
        elif out is not x:
            if not (_is_torch(out) and out.is_cuda and out.dtype == x.dtype and out.is_contiguous() and out.shape == x.shape
                    and out.device == x.device):
                raise TypeError("out must be a contiguous CUDA tensor of the input's shape, dtype and device")
        batch = x.numel() // self._n
        if batch:
            self.apply_ptr(x.data_ptr(), out.data_ptr(), batch, torch.cuda.current_stream(x.device).cuda_stream)
        return out

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            try:
                getattr(self._L, f"fourier_hip_conv_destroy_{self._suffix}")(h)
            except Exception:
                pass


def create_conv_f32(size, real_data=False, device=-1):
    return FftConv(size, "f32", real_data, device)


def create_conv_f64(size, real_data=False, device=-1):
    return FftConv(size, "f64", real_data, device)


_CONV_PLANS = {}


def fftconv(x, taps, correlate=False, out=None):
    """Circular convolution (or correlation) of the rows of a contiguous (..., N) CUDA tensor with `taps` of shape (taps,) or
    (F, taps) and the same dtype: complex64 / complex128 rows, or float32 / float64 rows (real data).  Handles are cached per
    (N, dtype, device) and the filters are set on EVERY call -- the slow way to apply the same filters repeatedly; keep an FftConv
    for that."""
    import torch

    kinds = {torch.complex64: ("f32", False), torch.complex128: ("f64", False), torch.float32: ("f32", True), torch.float64: ("f64", True)}
    if not (_is_torch(x) and x.is_cuda and x.dtype in kinds and x.is_contiguous()):
        raise TypeError("expected a contiguous CUDA complex64 / complex128 / float32 / float64 tensor")
    if x.dim() == 0:
        raise ValueError("expected at least one dimension")
    real, real_data = kinds[x.dtype]
    device = x.device.index if x.device.index is not None else torch.cuda.current_device()
    key = (int(x.shape[-1]), x.dtype, int(device))
    p = _CONV_PLANS.get(key)
    if p is None:
        p = _CONV_PLANS[key] = FftConv(x.shape[-1], real, real_data, device)
    p.set_filters(taps, correlate)
    return p.apply(x, out)


class RealFftN:
    """Batched real-input N-D transforms (include/fourier.h, fourier_hip_realnd_*) over items of `shape` (1 ... 4 dimensions, the
    last one real) on device memory, numpy's rfftn / irfftn layout: an item of reals has `shape`, an item of the half spectrum has
    shape[:-1] + (shape[-1]//2+1,).  Forward codes Fft / SqrtScaledFft, inverse codes Ifft / UnscaledIfft / SqrtScaledIfft, scaled
    over the product of the lengths."""

    def __init__(self, shape, real, device=-1):
        import ctypes

        self._suffix = {"f32": "float", "f64": "double"}[real]
        self.real = real
        self._L = _lib.lib()
        self.shape = tuple(int(n) for n in shape)
        dims = (ctypes.c_size_t * max(1, len(self.shape)))(*self.shape)
        self._h = getattr(self._L, f"fourier_hip_realnd_create_{self._suffix}")(len(self.shape), dims, int(device))
        if not self._h:
            raise FourierError(f"cannot create real N-D FFT plan of shape {self.shape}")

    def rank(self):
        return len(self.shape)

    def half_shape(self):
        return self.shape[:-1] + (self.shape[-1] // 2 + 1,)

    def describe(self):
        return getattr(self._L, f"fourier_hip_realnd_describe_{self._suffix}")(self._h).decode()

    def _check(self, st):
        if st != 0:
            raise FourierError(self._L.fourier_hip_status_string(st).decode())

    def forward_batch_ptr(self, d_in, d_out, batch, transform=Transform.Fft, stream=0):
        """`batch` items of reals at d_in -> `batch` items of the half spectrum at d_out, enqueued on `stream`."""
        self._check(getattr(self._L, f"fourier_hip_realnd_forward_batch_{self._suffix}")(
            self._h, d_in, d_out, int(batch), int(transform), stream))

    def inverse_batch_ptr(self, d_in, d_out, batch, transform=Transform.Ifft, stream=0):
        """`batch` items of the half spectrum at d_in -> `batch` items of reals at d_out (d_in is not modified)."""
        self._check(getattr(self._L, f"fourier_hip_realnd_inverse_batch_{self._suffix}")(
            self._h, d_in, d_out, int(batch), int(transform), stream))

    def reserve(self, batch):
        """Pre-size the plan-owned buffers: later calls of at most `batch` items never allocate."""
        self._check(getattr(self._L, f"fourier_hip_realnd_reserve_{self._suffix}")(self._h, int(batch)))

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            try:
                getattr(self._L, f"fourier_hip_realnd_destroy_{self._suffix}")(h)
            except Exception:
                pass


def set_default_option(key, value):
    """Library-wide default for plans created afterwards (include/fourier.h: fourier_hip_set_default_option), e.g.
    ("specialise_at_create", 2): lengths whose prime factors stop at 13 get their own kernels compiled inside create_fft_*."""
    if _lib.lib().fourier_hip_set_default_option(key.encode(), int(value)) != 0:
        raise FourierError(f"bad default option {key}={value}")


def get_default_option(key):
    return int(_lib.lib().fourier_hip_get_default_option(key.encode()))


def create_fft_f32(size, device=-1):
    """fourier/src/lib.rs:31-43."""
    return Fft(size, "f32", device)


def create_fft_f64(size, device=-1):
    """fourier/src/lib.rs:49-60."""
    return Fft(size, "f64", device)


_PLANS = {}


def _plan(n, real, device):
    """Plans of fftn / fft2, cached per (length, precision, device)."""
    key = (int(n), real, int(device))
    p = _PLANS.get(key)
    if p is None:
        p = _PLANS[key] = Fft(n, real, device)
    return p


def fftn(x, dims=None, transform=Transform.Fft, out=None):
    """N-dimensional transform of a contiguous CUDA complex64 / complex128 tensor over `dims` (default: all), one axis transform per
    dimension on the current stream.  Returns a new tensor, or `out` (which may be `x`).  Scaling per axis as numpy: Ifft is ifftn,
    the sqrt-scaled codes are norm="ortho"."""
    import torch

    if not (_is_torch(x) and x.is_cuda and x.dtype in (torch.complex64, torch.complex128) and x.is_contiguous()):
        raise TypeError("expected a contiguous CUDA complex64 / complex128 tensor")
    transform = Transform(transform)
    nd = x.dim()
    dims = tuple(range(nd)) if dims is None else tuple(dims)
    norm = []
    for d in dims:
        if not -nd <= d < nd:
            raise ValueError(f"dim {d} out of range for {nd} dimensions")
        norm.append(d % nd)
    if len(set(norm)) != len(norm):
        raise ValueError(f"repeated dimension in {dims}")
    if out is None:
        out = torch.empty_like(x)
    elif out is not x:
        if not (_is_torch(out) and out.is_cuda and out.dtype == x.dtype and out.is_contiguous() and out.shape == x.shape
                and out.device == x.device):
            raise TypeError("out must be a contiguous CUDA tensor of the input's shape, dtype and device")
    real = "f32" if x.dtype == torch.complex64 else "f64"
    device = x.device.index if x.device.index is not None else torch.cuda.current_device()
    src = x
    for d in norm:
        if x.shape[d] == 1:  # a 1-point transform is the identity under every code
            continue
        _plan(x.shape[d], real, device).transform_axis(src, out, transform, d)
        src = out
    if src is x and out is not x:  # every axis skipped
        out.copy_(x)
    return out


def fft2(x, transform=Transform.Fft, out=None):
    """fftn over the last two dimensions."""
    return fftn(x, (-2, -1), transform, out)


_REALND_PLANS = {}


def _realnd_plan(shape, real, device):
    """Plans of rfftn / irfftn, cached per (shape, precision, device)."""
    key = (tuple(int(n) for n in shape), real, int(device))
    p = _REALND_PLANS.get(key)
    if p is None:
        p = _REALND_PLANS[key] = RealFftN(key[0], real, device)
    return p


def realnd_layout(ndim, dims):
    """The `dims` of rfftn / irfftn on a tensor of `ndim` dimensions -> (dims normalised to 0 ... ndim-1, in the given order with
    the real axis last; perm), where perm is None if the transformed dimensions are the trailing block (in any order) with the real
    axis last, so that the plan runs on the tensor as it is, and otherwise the permutation (batch dimensions in order, then the
    transformed ones with the real axis last) that movedim applies before a contiguous copy (the slow case)."""
    dims = tuple(range(ndim)) if dims is None else tuple(dims)
    if not dims:
        raise ValueError("no dimension to transform")
    if len(dims) > 4:
        raise ValueError(f"at most 4 transformed dimensions, got {len(dims)}")
    norm = []
    for d in dims:
        d = int(d)
        if not -ndim <= d < ndim:
            raise ValueError(f"dim {d} out of range for {ndim} dimensions")
        norm.append(d % ndim)
    if len(set(norm)) != len(norm):
        raise ValueError(f"repeated dimension in {dims}")
    k = len(norm)
    if sorted(norm) == list(range(ndim - k, ndim)) and norm[-1] == ndim - 1:
        return tuple(norm), None
    batch = [d for d in range(ndim) if d not in norm]
    return tuple(norm), tuple(batch + sorted(norm[:-1]) + [norm[-1]])


def _realnd_run(x, dims, shape_of, forward, transform, out, out_dtype, real):
    """rfftn / irfftn behind the layout rule of realnd_layout: the plan of the transformed shape over the batch in front."""
    import torch

    norm, perm = realnd_layout(x.dim(), dims)
    src = x if perm is None else x.permute(perm).contiguous()
    k = len(norm)
    shape = shape_of(tuple(src.shape[src.dim() - k:]))  # the real-side shape of one item
    half = shape[:-1] + (shape[-1] // 2 + 1,)
    res_shape = tuple(src.shape[:src.dim() - k]) + (half if forward else shape)
    if perm is None:
        want = res_shape
    else:
        inv = [0] * len(perm)
        for i, d in enumerate(perm):
            inv[d] = i
        want = tuple(res_shape[inv[d]] for d in range(len(perm)))
    if out is not None and not (_is_torch(out) and out.is_cuda and out.dtype == out_dtype and out.is_contiguous()
                                and tuple(out.shape) == want and out.device == x.device):
        raise TypeError(f"out must be a contiguous CUDA {out_dtype} tensor of shape {want} on the input's device")
    res = out if (out is not None and perm is None) else torch.empty(res_shape, dtype=out_dtype, device=x.device)
    items = 1
    for n in src.shape[:src.dim() - k]:
        items *= n
    device = x.device.index if x.device.index is not None else torch.cuda.current_device()
    plan = _realnd_plan(shape, real, device)
    if items:
        stream = torch.cuda.current_stream(x.device).cuda_stream
        if forward:
            plan.forward_batch_ptr(src.data_ptr(), res.data_ptr(), items, transform, stream)
        else:
            plan.inverse_batch_ptr(src.data_ptr(), res.data_ptr(), items, transform, stream)
    if perm is None:
        return res
    back = res.permute(inv)
    if out is None:
        return back.contiguous()
    out.copy_(back)
    return out


def rfftn(x, dims=None, transform=Transform.Fft, out=None):
    """Real-input N-dimensional transform of a contiguous CUDA float32 / float64 tensor over `dims` (default: all, at most 4; the last
    entry is the real axis, whose length L becomes L//2+1), on the current stream, numpy's rfftn layout and scaling (SqrtScaledFft is
    norm="ortho").  Dimensions outside `dims` are the batch.  Returns a new complex tensor, or `out`.  When `dims` are not the trailing
    block with the real axis last, the input is permuted into a contiguous copy first and the result permuted back (slower)."""
    import torch

    if not (_is_torch(x) and x.is_cuda and x.dtype in (torch.float32, torch.float64) and x.is_contiguous()):
        raise TypeError("expected a contiguous CUDA float32 / float64 tensor")
    transform = Transform(transform)
    if not transform.is_forward():
        raise ValueError(f"{transform!r} is not a forward transform")
    real, cdt = ("f32", torch.complex64) if x.dtype == torch.float32 else ("f64", torch.complex128)
    return _realnd_run(x, dims, lambda s: s, True, transform, out, cdt, real)


def irfftn(X, dims=None, n=None, transform=Transform.Ifft, out=None):
    """Inverse of rfftn: a contiguous CUDA complex64 / complex128 half spectrum over `dims` (the last entry is the half-spectrum axis)
    -> reals, `n` (default 2 * (X.shape[last] - 1)) on the real axis, on the current stream.  numpy's irfftn scaling: Ifft is the
    default, SqrtScaledIfft is norm="ortho", UnscaledIfft is norm="forward".  Input that is not Hermitian gives numpy's result.
    X is not modified."""
    import torch

    if not (_is_torch(X) and X.is_cuda and X.dtype in (torch.complex64, torch.complex128) and X.is_contiguous()):
        raise TypeError("expected a contiguous CUDA complex64 / complex128 tensor")
    transform = Transform(transform)
    if transform.is_forward():
        raise ValueError(f"{transform!r} is not an inverse transform")
    real, rdt = ("f32", torch.float32) if X.dtype == torch.complex64 else ("f64", torch.float64)

    def shape_of(s):
        m = 2 * (s[-1] - 1) if n is None else int(n)
        if m < 1 or m // 2 + 1 != s[-1]:
            raise ValueError(f"real length {m} does not match {s[-1]} half-spectrum values")
        return s[:-1] + (m,)

    return _realnd_run(X, dims, shape_of, False, transform, out, rdt, real)


def rfft2(x, transform=Transform.Fft, out=None):
    """rfftn over the last two dimensions."""
    return rfftn(x, (-2, -1), transform, out)


def irfft2(X, n=None, transform=Transform.Ifft, out=None):
    """irfftn over the last two dimensions."""
    return irfftn(X, (-2, -1), n, transform, out)
