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
import ctypes
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


_SUFFIX = {"f32": "float", "f64": "double"}


def _torch_dtypes(real):
    """(real dtype, complex dtype) of a precision."""
    import torch

    return {"f32": (torch.float32, torch.complex64), "f64": (torch.float64, torch.complex128)}[real]


def _precision(dtype):
    """A torch dtype -> (precision, whether the dtype is the real one); None for any other dtype."""
    for real in _SUFFIX:
        if dtype in _torch_dtypes(real):
            return real, dtype == _torch_dtypes(real)[0]
    return None


def _names(dtypes):
    return " / ".join(str(d).replace("torch.", "") for d in dtypes)


def _is_cuda_tensor(x, dtypes):
    return _is_torch(x) and x.is_cuda and x.dtype in dtypes and x.is_contiguous()


def _require_cuda(x, *dtypes):
    if not _is_cuda_tensor(x, dtypes):
        raise TypeError(f"expected a contiguous CUDA {_names(dtypes)} tensor")


def _require_out(out, shape, dtype, device):
    if not (_is_cuda_tensor(out, (dtype,)) and tuple(out.shape) == tuple(shape) and out.device == device):
        raise TypeError(f"out must be a contiguous CUDA {_names((dtype,))} tensor of shape {tuple(shape)} on the input's device")


def _require_no_partial_overlap(input, output):
    """The same buffer is an in-place call; anything else must not overlap (include/fourier.h)."""
    a0, b0 = input.data_ptr(), output.data_ptr()
    nbytes = input.numel() * input.element_size()
    if a0 != b0 and a0 < b0 + nbytes and b0 < a0 + nbytes:
        raise ValueError("input and output overlap partially")


def _normalise_dims(ndim, dims):
    """`dims` (None: all) as a tuple of distinct indices in 0 ... ndim-1, in the given order."""
    dims = tuple(range(ndim)) if dims is None else tuple(dims)
    norm = []
    for d in dims:
        d = int(d)
        if not -ndim <= d < ndim:
            raise ValueError(f"dim {d} out of range for {ndim} dimensions")
        norm.append(d % ndim)
    if len(set(norm)) != len(norm):
        raise ValueError(f"repeated dimension in {dims}")
    return tuple(norm)


def _stream(x):
    import torch

    return torch.cuda.current_stream(x.device).cuda_stream


def _device_index(x):
    import torch

    return x.device.index if x.device.index is not None else torch.cuda.current_device()


def _raise_status(L, st, message=None):
    if st != 0:
        raise FourierError(message or L.fourier_hip_status_string(st).decode())


class _Handle:
    """A libfourier.so handle of one family: its entry points are <_prefix><op>_<float|double>."""

    _prefix = None
    _destroy = None  # the destroy symbol without the precision suffix

    def _create(self, real, what, *args):
        self._suffix = _SUFFIX[real]
        self.real = real
        self._L = _lib.lib()
        self._h = self._fn("create")(*args)
        if not self._h:
            # the reference's create panics -> NULL through the FFI (fourier-ffi/src/lib.rs:18-19)
            raise FourierError(f"cannot create {what}")

    def _fn(self, op):
        return getattr(self._L, f"{self._prefix}{op}_{self._suffix}")

    def _call(self, op, *args, message=None):
        _raise_status(self._L, self._fn(op)(self._h, *args), message)

    def describe(self):
        return self._fn("describe")(self._h).decode()

    def reserve(self, batch):
        """Pre-size the plan-owned buffers: later calls of at most `batch` rows (items) never allocate."""
        self._call("reserve", int(batch))

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            try:
                getattr(self._L, f"{self._destroy}_{self._suffix}")(h)
            except Exception:
                pass


class Fft(_Handle):
    """The `Fft` trait (fft.rs:40-82) over a libfourier.so plan handle."""

    _prefix = "fourier_hip_"
    _destroy = "fourier_destroy"

    def __init__(self, size, real, device=-1):
        self._create(real, f"FFT plan of size {size}", int(size), int(device))
        self.np_dtype = np.dtype(np.complex64 if real == "f32" else np.complex128)
        self._n = int(size)
        self.device = int(self._fn("device")(self._h))  # device=-1 binds the current one

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
        self._call("transform_batch", d_in, d_out, int(batch), int(transform), stream)

    def _require_numpy(self, *arrays):
        for a in arrays:
            if not (isinstance(a, np.ndarray) and a.dtype == self.np_dtype and a.flags.c_contiguous):
                raise TypeError(f"expected C-contiguous numpy {self.np_dtype} arrays")

    def transform_batch_host(self, input, output, transform):
        """`batch` contiguous transforms in host (numpy) memory, streamed through the device in chunks with
        copies and kernels overlapped; synchronous.  input may be output (in place)."""
        self._require_numpy(input, output)
        if input.size != output.size or input.size % self._n != 0:
            raise ValueError(f"buffers of {input.size}/{output.size} elements are not the same whole number of transforms")
        self._call("transform_batch_host", input.ctypes.data, output.ctypes.data, input.size // self._n, int(transform))

    def synchronize(self, stream=0):
        """Blocks until everything queued on `stream` (a HIP stream handle, 0 = the NULL stream) of the plan's device has
        finished: the wait that follows a stream-ordered transform_batch_ptr when no other runtime owns the stream."""
        self._call("synchronize", stream)

    def reserve(self, batch, in_place=False):
        """Pre-size the plan-owned device buffers so that later batched calls of up to `batch` transforms never
        allocate (hipMalloc synchronises the device; needed before HIP-graph capture)."""
        self._call("reserve", int(batch), int(bool(in_place)))

    def profile_batch_ptr(self, d_in, d_out, batch, transform, stream=0, nslots=16):
        """One batched transform with a HIP event pair around every kernel launch.
        Returns [(slot_name, total_ms, launches), ...] in launch order."""
        import ctypes

        ms = (ctypes.c_float * nslots)()
        cnt = (ctypes.c_int * nslots)()
        self._call("profile", d_in, d_out, int(batch), int(transform), stream, nslots, ms, cnt)
        names = self._fn("slot_names")(self._h).decode().split(",")
        return [(nm, float(ms[i]), int(cnt[i])) for i, nm in enumerate(names) if i < nslots]

    def set_option(self, key, value):
        self._call("set_option", key.encode(), int(value), message=f"bad option {key}={value}")

    def model_bytes(self):
        return self._fn("model_bytes")(self._h)

    # -- transforms along a strided axis (extension) -----------------------------------------
    def transform_axis_ptr(self, d_in, d_out, outer, inner, transform, stream=0):
        """Raw-pointer form: the middle axis of an [outer][size][inner] complex array on device memory, enqueued on `stream`."""
        self._call("transform_axis", d_in, d_out, int(outer), int(inner), int(transform), stream)

    def reserve_axis(self, outer, inner):
        """Pre-size the plan-owned buffers so that later axis calls of at most outer x inner never allocate."""
        self._call("reserve_axis", int(outer), int(inner))

    def describe_axis(self, inner):
        """The route an axis call with this `inner` takes (include/fourier.h)."""
        return self._fn("describe_axis")(self._h, int(inner)).decode()

    def _require_on_device(self, *tensors):
        """The plan's tables, scratch and kernels live on ONE device (fixed at creation)."""
        for t in tensors:
            if t.device.index != self.device:
                raise ValueError(f"tensor on cuda:{t.device.index}, plan on cuda:{self.device}")

    def transform_axis(self, input, output, transform, dim):
        """Transform contiguous CUDA complex tensors along dimension `dim` (shape[dim] == size()), on the current stream.
        input may be output (in place); any other overlap is refused."""
        for t in (input, output):
            _require_cuda(t, _torch_dtypes(self.real)[1])
            self._require_on_device(t)
        if input.shape != output.shape:
            raise ValueError(f"shapes {tuple(input.shape)} and {tuple(output.shape)} differ")
        dim, = _normalise_dims(input.dim(), (dim,))
        if input.shape[dim] != self._n:
            raise ValueError(f"dimension {dim} has {input.shape[dim]} elements, plan size is {self._n}")
        _require_no_partial_overlap(input, output)
        outer = 1
        for d in input.shape[:dim]:
            outer *= d
        inner = 1
        for d in input.shape[dim + 1:]:
            inner *= d
        if outer * inner == 0:
            return
        self.transform_axis_ptr(input.data_ptr(), output.data_ptr(), outer, inner, int(transform), _stream(input))

    # -- plumbing --------------------------------------------------------------------------
    def _dispatch(self, input, output, transform):
        code = int(transform)
        if _is_torch(input) or _is_torch(output):
            for t in (input, output):
                _require_cuda(t, _torch_dtypes(self.real)[1])
            # the reference asserts input.len() == output.len() == size (fft.rs:57-58); the batched
            # extension accepts any whole number of transforms
            if input.numel() != output.numel() or input.numel() % self._n != 0 or input.numel() == 0:
                raise ValueError(f"buffer of {input.numel()} elements is not a multiple of size {self._n}")
            self._require_on_device(input, output)
            _require_no_partial_overlap(input, output)
            self.transform_batch_ptr(input.data_ptr(), output.data_ptr(), input.numel() // self._n, code, _stream(input))
            return
        self._require_numpy(input, output)
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
        _raise_status(self._L, self._fn("last_status")(self._h))


class _RealHandle(_Handle):
    """What the two real-input families share: rows (items) of reals <-> rows (items) of the half spectrum."""

    def forward_batch_ptr(self, d_in, d_out, batch, transform=Transform.Fft, stream=0):
        """`batch` rows (items) of reals at d_in -> `batch` rows (items) of the half spectrum at d_out, enqueued on `stream`."""
        self._call("forward_batch", d_in, d_out, int(batch), int(transform), stream)

    def inverse_batch_ptr(self, d_in, d_out, batch, transform=Transform.Ifft, stream=0):
        """`batch` rows (items) of the half spectrum at d_in -> `batch` rows (items) of reals at d_out (d_in is not modified)."""
        self._call("inverse_batch", d_in, d_out, int(batch), int(transform), stream)


class RealFft(_RealHandle):
    """Batched real-input transforms (include/fourier.h, fourier_hip_real_*): N reals per row <-> N//2+1 complex per row, numpy's
    rfft / irfft layout, on device memory.  Forward codes Fft / SqrtScaledFft, inverse codes Ifft / UnscaledIfft / SqrtScaledIfft."""

    _prefix = "fourier_hip_real_"
    _destroy = "fourier_hip_real_destroy"

    def __init__(self, size, real, device=-1):
        self._create(real, f"real FFT plan of size {size}", int(size), int(device))
        self._n = int(size)

    def size(self):
        return self._n

    def _run(self, x, side, run, transform):
        """One side's contiguous (..., last) CUDA tensor through `run` into a new tensor of the other side, on the current stream."""
        import torch

        lengths = (self._n, self._n // 2 + 1)
        _require_cuda(x, _torch_dtypes(self.real)[side])
        if x.dim() == 0 or x.shape[-1] != lengths[side]:
            raise ValueError(f"last dimension must be {lengths[side]}, got {tuple(x.shape)}")
        out = torch.empty(x.shape[:-1] + (lengths[1 - side],), dtype=_torch_dtypes(self.real)[1 - side], device=x.device)
        batch = x.numel() // lengths[side]
        if batch:
            run(x.data_ptr(), out.data_ptr(), batch, transform, _stream(x))
        return out

    def rfft(self, x, transform=Transform.Fft):
        """Contiguous (..., N) float32 / float64 CUDA tensor -> new (..., N//2+1) complex tensor, on the current stream."""
        return self._run(x, 0, self.forward_batch_ptr, transform)

    def irfft(self, X, transform=Transform.Ifft):
        """Contiguous (..., N//2+1) complex CUDA tensor -> new (..., N) real tensor, on the current stream; X is not modified."""
        return self._run(X, 1, self.inverse_batch_ptr, transform)


def create_rfft_f32(size, device=-1):
    return RealFft(size, "f32", device)


def create_rfft_f64(size, device=-1):
    return RealFft(size, "f64", device)


class FftConv(_Handle):
    """Batched circular convolution / correlation with a prepared filter bank (include/fourier.h, fourier_hip_conv_*) on device
    memory: rows of N complex values (real_data=False) or N reals (real_data=True) in, rows of the same shape out, row b with filter
    b mod F.  The filters are given in the time domain (set_filters) and transformed once."""

    _prefix = "fourier_hip_conv_"
    _destroy = "fourier_hip_conv_destroy"

    def __init__(self, size, real, real_data=False, device=-1):
        self.real_data = bool(real_data)
        self._create(real, f"convolution plan of size {size}", int(size), int(self.real_data), int(device))
        self._n = int(size)

    def size(self):
        return self._n

    def filters(self):
        return int(self._fn("filters")(self._h))

    def set_option(self, key, value):
        """"fusion": 1 (default) / 0 = the composed route (forward transform, product sweep, inverse transform)."""
        self._call("set_option", key.encode(), int(value))

    def set_filters_ptr(self, d_taps, taps, filters=1, correlate=False, stream=0):
        """`filters` rows of `taps` values of the handle's kind at d_taps -> the bank, enqueued on `stream`."""
        self._call("set_filters", d_taps, int(taps), int(filters), int(bool(correlate)), stream)

    def apply_ptr(self, d_in, d_out, batch, stream=0):
        """`batch` rows of N values at d_in -> `batch` rows at d_out (d_out may be d_in), enqueued on `stream`."""
        self._call("apply", d_in, d_out, int(batch), stream)

    def _dtype(self):
        return _torch_dtypes(self.real)[0 if self.real_data else 1]

    def set_filters(self, taps, correlate=False):
        """Contiguous CUDA tensor of shape (taps,) or (F, taps), of the handle's dtype, 1 <= taps <= N; on the current stream."""
        _require_cuda(taps, self._dtype())
        if taps.dim() not in (1, 2) or taps.numel() == 0 or taps.shape[-1] > self._n:
            raise ValueError(f"taps must have shape (taps,) or (F, taps) with 1 <= taps <= {self._n}, got {tuple(taps.shape)}")
        self.set_filters_ptr(taps.data_ptr(), taps.shape[-1], taps.numel() // taps.shape[-1], correlate, _stream(taps))

    def apply(self, x, out=None):
        """Contiguous (..., N) CUDA tensor of the handle's dtype -> a new tensor of the same shape, or `out` (which may be `x`), on
        the current stream.  Row b of the flattened leading dimensions uses filter b mod F."""
        import torch

        _require_cuda(x, self._dtype())
        if x.dim() == 0 or x.shape[-1] != self._n:
            raise ValueError(f"last dimension must be {self._n}, got {tuple(x.shape)}")
        if out is None:
            out = torch.empty_like(x)
        elif out is not x:
            _require_out(out, x.shape, x.dtype, x.device)
        batch = x.numel() // self._n
        if batch:
            self.apply_ptr(x.data_ptr(), out.data_ptr(), batch, _stream(x))
        return out


def create_conv_f32(size, real_data=False, device=-1):
    return FftConv(size, "f32", real_data, device)


def create_conv_f64(size, real_data=False, device=-1):
    return FftConv(size, "f64", real_data, device)


_PLANS = {}


def _cached_plan(cls, *args):
    """The handles behind fftn, rfftn / irfftn and fftconv, cached per (class, constructor arguments)."""
    key = (cls,) + args
    p = _PLANS.get(key)
    if p is None:
        p = _PLANS[key] = cls(*args)
    return p


def fftconv(x, taps, correlate=False, out=None):
    """Circular convolution (or correlation) of the rows of a contiguous (..., N) CUDA tensor with `taps` of shape (taps,) or
    (F, taps) and the same dtype: complex64 / complex128 rows, or float32 / float64 rows (real data).  Handles are cached per
    (N, dtype, device) and the filters are set on EVERY call -- the slow way to apply the same filters repeatedly; keep an FftConv
    for that."""
    _require_cuda(x, *_torch_dtypes("f32"), *_torch_dtypes("f64"))
    if x.dim() == 0:
        raise ValueError("expected at least one dimension")
    real, real_data = _precision(x.dtype)
    p = _cached_plan(FftConv, int(x.shape[-1]), real, real_data, int(_device_index(x)))
    p.set_filters(taps, correlate)
    return p.apply(x, out)


LCONV_MODES = {"full": 0, "same": 1, "valid": 2}  # FOURIER_LCONV_FULL ... FOURIER_LCONV_VALID


class LinearConv(_Handle):
    """Batched linear convolution / correlation with a prepared filter bank (include/fourier.h, fourier_hip_lconv_*) on device memory:
    rows of `length` values in, rows of out_length() values out ("full", "same", "valid" as numpy.convolve), row b with filter b mod F;
    complex rows with complex taps (real_data=False) or real rows with real taps (real_data=True).  The filters are given in the time
    domain (set_filters) and transformed once."""

    _prefix = "fourier_hip_lconv_"
    _destroy = "fourier_hip_lconv_destroy"

    def __init__(self, length, taps, real="f32", mode="full", real_data=False, device=-1):
        if mode not in LCONV_MODES:
            raise ValueError(f"mode must be one of {sorted(LCONV_MODES)}, got {mode!r}")
        self.real_data = bool(real_data)
        self.mode = mode
        self._create(real, f"linear convolution plan of length {length}, {taps} taps, mode {mode}", int(length), int(taps),
                     LCONV_MODES[mode], int(self.real_data), int(device))
        self._lx, self._k = int(length), int(taps)
        self._lout = int(self._fn("out_length")(self._h))

    def length(self):
        return self._lx

    def taps(self):
        return self._k

    def out_length(self):
        return self._lout

    def filters(self):
        return int(self._fn("filters")(self._h))

    def set_option(self, key, value):
        """"block": 11 ... 15 forces the overlap-save block 2^value, 0 = the rule; "overlap_save": 0 = the padded route, 1 (default).
        A change of route or block drops the bank: set the filters again."""
        self._call("set_option", key.encode(), int(value))

    def set_filters_ptr(self, d_taps, filters=1, correlate=False, stream=0):
        """`filters` rows of taps() values of the handle's kind at d_taps -> the bank, enqueued on `stream`."""
        self._call("set_filters", d_taps, int(filters), int(bool(correlate)), stream)

    def apply_ptr(self, d_in, d_out, batch, stream=0):
        """`batch` rows of length() values at d_in -> `batch` rows of out_length() values at d_out (no overlap), enqueued on `stream`."""
        self._call("apply", d_in, d_out, int(batch), stream)

    def _dtype(self):
        return _torch_dtypes(self.real)[0 if self.real_data else 1]

    def set_filters(self, taps, correlate=False):
        """Contiguous CUDA tensor of shape (K,) or (F, K), of the handle's dtype; on the current stream."""
        _require_cuda(taps, self._dtype())
        if taps.dim() not in (1, 2) or taps.numel() == 0 or taps.shape[-1] != self._k:
            raise ValueError(f"taps must have shape ({self._k},) or (F, {self._k}), got {tuple(taps.shape)}")
        self.set_filters_ptr(taps.data_ptr(), taps.numel() // self._k, correlate, _stream(taps))

    def apply(self, x, out=None):
        """Contiguous (..., length) CUDA tensor of the handle's dtype -> a new (..., out_length) tensor, or `out` (which may not
        overlap `x`), on the current stream.  Row b of the flattened leading dimensions uses filter b mod F."""
        import torch

        _require_cuda(x, self._dtype())
        if x.dim() == 0 or x.shape[-1] != self._lx:
            raise ValueError(f"last dimension must be {self._lx}, got {tuple(x.shape)}")
        shape = tuple(x.shape[:-1]) + (self._lout,)
        if out is None:
            out = torch.empty(shape, dtype=x.dtype, device=x.device)
        else:
            _require_out(out, shape, x.dtype, x.device)
        batch = x.numel() // self._lx
        if batch:
            self.apply_ptr(x.data_ptr(), out.data_ptr(), batch, _stream(x))
        return out


def create_lconv_f32(length, taps, mode="full", real_data=False, device=-1):
    return LinearConv(length, taps, "f32", mode, real_data, device)


def create_lconv_f64(length, taps, mode="full", real_data=False, device=-1):
    return LinearConv(length, taps, "f64", mode, real_data, device)


def fftconvolve(x, taps, mode="full", correlate=False, out=None):
    """Linear convolution (or correlation) of the rows of a contiguous (..., Lx) CUDA tensor with `taps` of shape (K,) or (F, K) and
    the same dtype, numpy.convolve's "full" / "same" / "valid" (numpy.correlate's with correlate=True): complex64 / complex128 rows, or
    float32 / float64 rows (real data).  Handles are cached per (Lx, K, dtype, mode, device) and the filters are set on EVERY call; keep
    a LinearConv to apply the same filters repeatedly."""
    _require_cuda(x, *_torch_dtypes("f32"), *_torch_dtypes("f64"))
    if x.dim() == 0:
        raise ValueError("expected at least one dimension")
    if not _is_torch(taps) or taps.dim() not in (1, 2) or taps.numel() == 0:
        raise TypeError("taps must be a tensor of shape (K,) or (F, K)")
    real, real_data = _precision(x.dtype)
    p = _cached_plan(LinearConv, int(x.shape[-1]), int(taps.shape[-1]), real, mode, real_data, int(_device_index(x)))
    p.set_filters(taps, correlate)
    return p.apply(x, out)


class FftConvNd(_Handle):
    """Batched N-D circular convolution / correlation of REAL items with a prepared filter bank (include/fourier.h,
    fourier_hip_convnd_*) on device memory, over the trailing len(shape) = 2, 3 or 4 dimensions.  `shape` is the transform shape S:
    items of in_shape <= S are zero-extended to S, convolved circularly with filter (filter_first + b) mod F, and the window
    [out_first, out_first + out_shape) is stored (set_window; the default is S, 0, S).  The filters are given in the time domain
    (set_filters) and transformed once.  Rank 1 is FftConv(real_data=True)."""

    _prefix = "fourier_hip_convnd_"
    _destroy = "fourier_hip_convnd_destroy"

    def __init__(self, shape, real="f32", device=-1):
        shape = tuple(int(n) for n in shape)
        if not 2 <= len(shape) <= 4 or any(n < 1 for n in shape):
            raise ValueError(f"shape must have 2 to 4 lengths >= 1 (rank 1 is FftConv), got {shape}")
        self._shape = shape
        self._create(real, f"N-D convolution plan of shape {shape}", len(shape), self._sizes(shape), int(device))
        self._in, self._first, self._out = shape, (0,) * len(shape), shape

    @staticmethod
    def _sizes(values):
        return (ctypes.c_size_t * len(values))(*values)

    def shape(self):
        return self._shape

    def filters(self):
        return int(self._fn("filters")(self._h))

    def set_option(self, key, value):
        """"fusion": 1 = the fused untangle route where the last length is even, 0 = the composed route (rfftn, product sweep, irfftn)."""
        self._call("set_option", key.encode(), int(value))

    def set_filters_ptr(self, d_taps, taps_shape, filters=1, correlate=False, stream=0):
        """`filters` contiguous blocks of taps_shape <= S reals at d_taps -> the bank, enqueued on `stream`."""
        taps_shape = tuple(int(n) for n in taps_shape)
        if len(taps_shape) != len(self._shape):
            raise ValueError(f"taps_shape must have {len(self._shape)} lengths, got {taps_shape}")
        self._call("set_filters", d_taps, self._sizes(taps_shape), int(filters), int(bool(correlate)), stream)

    def set_window(self, in_shape=None, out_first=None, out_shape=None):
        """The extent of the items read (zero-extended to S at the high end) and the window of the circular result stored; None is the
        default of each (S, 0, S).  Host state: takes effect from the next apply."""
        r = len(self._shape)
        win = [tuple(int(n) for n in (d if v is None else v)) for v, d in ((in_shape, self._shape), (out_first, (0,) * r), (out_shape, self._shape))]
        if any(len(v) != r or any(n < 0 for n in v) for v in win):
            raise ValueError(f"in_shape, out_first and out_shape must have {r} non-negative lengths")
        self._call("set_window", *(self._sizes(v) for v in win))
        self._in, self._first, self._out = win

    def apply_ptr(self, d_in, d_out, batch, filter_first=0, stream=0):
        """`batch` items of in_shape reals at d_in -> `batch` items of out_shape reals at d_out, enqueued on `stream`."""
        self._call("apply_batch", d_in, d_out, int(batch), int(filter_first), stream)

    def _dtype(self):
        return _torch_dtypes(self.real)[0]

    def set_filters(self, taps, correlate=False):
        """Contiguous CUDA tensor of shape k or (F,) + k with k <= S in every dimension, of the handle's real dtype; on the current stream."""
        r = len(self._shape)
        _require_cuda(taps, self._dtype())
        k = tuple(taps.shape[-r:])
        if taps.dim() not in (r, r + 1) or taps.numel() == 0 or any(a > n for a, n in zip(k, self._shape)):
            raise ValueError(f"taps must have shape k or (F,) + k with 1 <= k <= {self._shape}, got {tuple(taps.shape)}")
        self.set_filters_ptr(taps.data_ptr(), k, taps.shape[0] if taps.dim() == r + 1 else 1, correlate, _stream(taps))

    def apply(self, x, filter_first=0, out=None):
        """Contiguous (..., *in_shape) CUDA tensor of the handle's real dtype -> a new (..., *out_shape) tensor, or `out` (which may be
        `x` under the default window, and may not overlap it otherwise), on the current stream.  Item b of the flattened leading
        dimensions uses filter (filter_first + b) mod F."""
        import torch

        r = len(self._shape)
        _require_cuda(x, self._dtype())
        if x.dim() < r or tuple(x.shape[-r:]) != self._in:
            raise ValueError(f"the last {r} dimensions must be {self._in}, got {tuple(x.shape)}")
        if int(filter_first) < 0:
            raise ValueError("filter_first must not be negative")
        shape = tuple(x.shape[:-r]) + self._out
        if out is None:
            out = torch.empty(shape, dtype=x.dtype, device=x.device)
        elif out is not x or shape != tuple(x.shape):
            _require_out(out, shape, x.dtype, x.device)
        batch = 1
        for n in x.shape[:-r]:
            batch *= int(n)
        if batch:
            self.apply_ptr(x.data_ptr(), out.data_ptr(), batch, filter_first, _stream(x))
        return out


def create_convnd_f32(shape, device=-1):
    return FftConvNd(shape, "f32", device)


def create_convnd_f64(shape, device=-1):
    return FftConvNd(shape, "f64", device)


def next_fast_len(n, even=False):
    """The smallest m >= n of the form 2^a 3^b 5^c 7^d (with even=True: the smallest even one), the padded length fftconvolven picks
    per dimension.  An UNMEASURED heuristic: lengths of small prime factors run on the mixed-radix and register-stage plans, but no
    measurement ranks the candidates; pass `shape=` where a measured length is known."""
    m = max(int(n), 1)
    if even and m % 2:
        m += 1
    while True:
        rest = m
        for p in (2, 3, 5, 7):
            while rest % p == 0:
                rest //= p
        if rest == 1:
            return m
        m += 2 if even else 1


def _convnd_run(x, taps, dims, r, correlate, window, out):
    """The N-D handle of the transform shape window[0] over the `dims` of x (None: the trailing r), cached per (shape, dtype, device);
    filters and window are set on every call."""
    shape, in_shape, first, out_shape = window
    real = _precision(x.dtype)[0]
    if dims is None:
        perm = None
    else:
        norm = _normalise_dims(x.dim(), dims)
        perm = None if norm == tuple(range(x.dim() - r, x.dim())) else tuple(d for d in range(x.dim()) if d not in norm) + norm
    src = x if perm is None else x.permute(perm).contiguous()
    p = _cached_plan(FftConvNd, tuple(shape), real, int(_device_index(x)))
    p.set_window(in_shape, first, out_shape)
    p.set_filters(taps, correlate)
    if perm is None:
        return p.apply(src, 0, out)
    inv = [0] * len(perm)
    for i, d in enumerate(perm):
        inv[d] = i
    back = p.apply(src).permute(inv)
    if out is None:
        return back.contiguous()
    _require_out(out, tuple(back.shape), x.dtype, x.device)
    out.copy_(back)
    return out


def _convnd_taps(x, taps, r):
    _require_cuda(x, _torch_dtypes("f32")[0], _torch_dtypes("f64")[0])
    if not 2 <= r <= 4 or x.dim() < r:
        raise ValueError(f"2 to 4 transformed dimensions of a tensor that has them, got {r} of {x.dim()}")
    if not _is_torch(taps) or taps.dim() not in (r, r + 1) or taps.numel() == 0:
        raise TypeError(f"taps must be a tensor of shape k or (F,) + k with {r} lengths in k")
    return tuple(int(n) for n in taps.shape[-r:])


def fftconvn(x, taps, dims=None, correlate=False, out=None):
    """Circular convolution (or correlation) of a contiguous CUDA float32 / float64 tensor over `dims` with real `taps` of the same
    dtype and shape k or (F,) + k, k <= the lengths of `dims`; dimensions outside `dims` are the batch, item b with filter b mod F.
    dims=None means the trailing taps.dim() dimensions and one filter (give `dims` for a bank).  Two to four dimensions; one is
    fftconv.  Dimensions that are not the trailing block in order are permuted into a contiguous copy first (slower).  Handles are
    cached per (shape, dtype, device) and the filters are set on EVERY call; keep an FftConvNd to apply the same filters repeatedly."""
    r = taps.dim() if dims is None else len(tuple(dims))
    _convnd_taps(x, taps, r)
    norm = tuple(range(x.dim() - r, x.dim())) if dims is None else _normalise_dims(x.dim(), dims)
    shape = tuple(int(x.shape[d]) for d in norm)
    return _convnd_run(x, taps, dims, r, correlate, (shape, shape, (0,) * r, shape), out)


def fftconv2(x, taps, correlate=False, out=None):
    """fftconvn over the last two dimensions; taps of shape (k1, k2) or (F, k1, k2)."""
    return fftconvn(x, taps, (-2, -1), correlate, out)


def fftconvolven(x, taps, mode="full", correlate=False, shape=None, out=None, rank=None):
    """Linear convolution of a contiguous CUDA float32 / float64 tensor over its trailing `rank` dimensions (default: taps.dim(), one
    filter; give `rank` for a bank) with real `taps` of shape k or (F,) + k, as scipy.signal.convolve over those dimensions: with
    items of shape a, "full" is a + k - 1 values per dimension, "same" the a values from (k - 1) // 2 on, "valid" the a - k + 1 values
    from k - 1 on (a >= k in every dimension).  correlate=True flips the taps along every transformed dimension and convolves, which
    is scipy.signal.correlate for real data.  The transform shape is next_fast_len(a + k - 1) per dimension, even in the last one so
    that the fused route exists, or `shape` (>= a + k - 1 in every dimension).  Handles are cached per (shape, dtype, device) and
    the filters are set on EVERY call; keep an FftConvNd to apply the same filters repeatedly."""
    import torch

    if mode not in LCONV_MODES:
        raise ValueError(f"mode must be one of {sorted(LCONV_MODES)}, got {mode!r}")
    r = int(rank) if rank is not None else (len(tuple(shape)) if shape is not None else (taps.dim() if _is_torch(taps) else 0))
    k = _convnd_taps(x, taps, r)
    a = tuple(int(n) for n in x.shape[-r:])
    full = tuple(n + m - 1 for n, m in zip(a, k))
    if mode == "valid" and any(n < m for n, m in zip(a, k)):
        raise ValueError(f"mode 'valid' needs items of at least the taps' shape {k} in every dimension, got {a}")
    if shape is None:
        shape = tuple(next_fast_len(n, even=(d == r - 1)) for d, n in enumerate(full))
    shape = tuple(int(n) for n in shape)
    if len(shape) != r or any(s < n for s, n in zip(shape, full)):
        raise ValueError(f"shape must have {r} lengths of at least {full}, got {shape}")
    first = {"full": (0,) * r, "same": tuple((m - 1) // 2 for m in k), "valid": tuple(m - 1 for m in k)}[mode]
    size = {"full": full, "same": a, "valid": tuple(n - m + 1 for n, m in zip(a, k))}[mode]
    if correlate:
        taps = torch.flip(taps, tuple(range(-r, 0))).contiguous()
    return _convnd_run(x, taps, None, r, False, (shape, a, first, size), out)


def fftconvolve2(x, taps, mode="full", correlate=False, shape=None, out=None):
    """fftconvolven over the last two dimensions; taps of shape (k1, k2) or (F, k1, k2)."""
    return fftconvolven(x, taps, mode, correlate, shape, out, rank=2)


R2R_KINDS = {("dct", 2): 0, ("dct", 3): 1, ("dst", 2): 2, ("dst", 3): 3}  # FOURIER_R2R_DCT2 ... FOURIER_R2R_DST3
R2R_NORMS = {None: 0, "backward": 0, "ortho": 1, "forward": 2}             # FOURIER_R2R_NORM_*


class R2R(_Handle):
    """Batched DCT / DST of types II and III (include/fourier.h, fourier_hip_r2r_*) on device memory: rows of N reals in, rows of N
    reals out, scipy.fft's definitions and norms.  One handle serves every kind and norm."""

    _prefix = "fourier_hip_r2r_"
    _destroy = "fourier_hip_r2r_destroy"

    def __init__(self, size, real, device=-1):
        self._create(real, f"real-to-real plan of size {size}", int(size), int(device))
        self._n = int(size)

    def size(self):
        return self._n

    def transform_batch_ptr(self, d_in, d_out, batch, kind, norm=0, stream=0):
        """`batch` rows of N reals at d_in -> `batch` rows at d_out (d_out may be d_in), enqueued on `stream`; kind and norm are the
        header's FOURIER_R2R_* values (R2R_KINDS, R2R_NORMS)."""
        self._call("transform_batch", d_in, d_out, int(batch), int(kind), int(norm), stream)

    def transform(self, x, kind, norm=0, out=None):
        """Contiguous (..., N) float32 / float64 CUDA tensor -> a new tensor of the same shape, or `out` (which may be `x`), on the
        current stream."""
        import torch

        _require_cuda(x, _torch_dtypes(self.real)[0])
        if x.dim() == 0 or x.shape[-1] != self._n:
            raise ValueError(f"last dimension must be {self._n}, got {tuple(x.shape)}")
        if out is None:
            out = torch.empty_like(x)
        elif out is not x:
            _require_out(out, x.shape, x.dtype, x.device)
            _require_no_partial_overlap(x, out)
        batch = x.numel() // self._n
        if batch:
            self.transform_batch_ptr(x.data_ptr(), out.data_ptr(), batch, kind, norm, _stream(x))
        return out


def create_r2r_f32(size, device=-1):
    return R2R(size, "f32", device)


def create_r2r_f64(size, device=-1):
    return R2R(size, "f64", device)


def _r2r(family, inverse, x, type, norm, dim, out):
    import torch

    if type not in (2, 3):
        raise ValueError(f"{family} type {type!r} is not supported: types 2 and 3 are (types 1 and 4 are unsupported)")
    if norm not in R2R_NORMS:
        raise ValueError(f"norm must be None, 'backward', 'ortho' or 'forward', got {norm!r}")
    if not (_is_torch(x) and x.is_cuda and x.dtype in (torch.float32, torch.float64)):
        raise TypeError("expected a CUDA float32 / float64 tensor")
    if x.dim() == 0:
        raise ValueError("expected at least one dimension")
    d = _normalise_dims(x.dim(), (dim,))[0]
    if x.shape[d] == 0:
        raise ValueError(f"the transformed dimension must have length >= 1, got {tuple(x.shape)}")
    code = R2R_NORMS[norm]
    if inverse:  # scipy's idct / idst: the other type, backward and forward exchanged
        type, code = 5 - type, {0: 2, 1: 1, 2: 0}[code]
    kind = R2R_KINDS[(family, type)]
    if out is not None and out is not x:
        if not (_is_torch(out) and out.is_cuda and out.dtype == x.dtype and tuple(out.shape) == tuple(x.shape) and out.device == x.device):
            raise TypeError(f"out must be a CUDA {_names((x.dtype,))} tensor of shape {tuple(x.shape)} on the input's device")
    plan = _cached_plan(R2R, int(x.shape[d]), _precision(x.dtype)[0], int(_device_index(x)))
    last = d == x.dim() - 1
    if last and x.is_contiguous() and (out is None or out.is_contiguous()):
        return plan.transform(x, kind, code, out)
    # any other dim (or layout): a torch copy that makes the axis last and contiguous, the transform in place there, a copy back
    work = x.movedim(d, -1).contiguous()
    if work.data_ptr() == x.data_ptr():
        work = work.clone()
    plan.transform(work, kind, code, work)
    res = work.movedim(-1, d)
    if out is None:
        return res.contiguous()
    out.copy_(res)
    return out


def dct(x, type=2, norm=None, dim=-1, out=None):
    """scipy.fft.dct of a float32 / float64 CUDA tensor along `dim`, types 2 and 3 (types 1 and 4 raise ValueError), norm None /
    "backward" / "ortho" / "forward" (scipy's orthogonalised "ortho"), on the current stream; returns a new tensor or `out`, which
    may be `x`.  Only the last dimension of a contiguous tensor is native (one cached R2R handle per (N, dtype, device)); any other
    `dim` is moved last with a torch copy, transformed there and moved back."""
    return _r2r("dct", False, x, type, norm, dim, out)


def idct(x, type=2, norm=None, dim=-1, out=None):
    """scipy.fft.idct: the inverse of dct(type, norm) -- the other type with "backward" and "forward" exchanged.  See dct."""
    return _r2r("dct", True, x, type, norm, dim, out)


def dst(x, type=2, norm=None, dim=-1, out=None):
    """scipy.fft.dst, types 2 and 3.  See dct."""
    return _r2r("dst", False, x, type, norm, dim, out)


def idst(x, type=2, norm=None, dim=-1, out=None):
    """scipy.fft.idst: the inverse of dst(type, norm).  See dct."""
    return _r2r("dst", True, x, type, norm, dim, out)


STFT_PAD_MODES = {"none": 0, "reflect": 1, "constant": 2}  # FOURIER_STFT_PAD_NONE / _REFLECT / _ZERO; "none" is center=False


def _stft_pad_mode(center, pad_mode):
    if not center:
        return "none"
    if pad_mode not in ("reflect", "constant"):
        raise ValueError(f"pad_mode must be 'reflect' or 'constant', got {pad_mode!r}")
    return pad_mode


class Stft(_Handle):
    """Batched short-time Fourier transform and its inverse (include/fourier.h, fourier_hip_stft_*) on device memory, torch.stft /
    torch.istft with onesided=True: rows of `length` reals <-> frames x bins complex per row, FRAME-MAJOR (frame f of row b at complex
    offset (b * frames + f) * bins).  n_fft, hop, win_length and the padding are fixed at create; the window is set afterwards
    (set_window; default all ones)."""

    _prefix = "fourier_hip_stft_"
    _destroy = "fourier_hip_stft_destroy"

    def __init__(self, n_fft, real="f32", hop_length=None, win_length=None, center=True, pad_mode="reflect", device=-1):
        n_fft = int(n_fft)
        hop = n_fft // 4 if hop_length is None else int(hop_length)
        wl = n_fft if win_length is None else int(win_length)
        self.pad_mode = _stft_pad_mode(center, pad_mode)
        if n_fft < 1 or hop < 1 or not 1 <= wl <= n_fft:
            raise ValueError(f"need n_fft >= 1, hop_length >= 1 and 1 <= win_length <= n_fft, got {n_fft}, {hop}, {wl}")
        self._create(real, f"STFT plan of n_fft {n_fft}, hop {hop}, win_length {wl}, padding {self.pad_mode}", n_fft, hop, wl,
                     STFT_PAD_MODES[self.pad_mode], int(device))
        self._n, self._hop, self._wl = n_fft, hop, wl
        self._pad = 0 if self.pad_mode == "none" else n_fft // 2

    def n_fft(self):
        return self._n

    def hop(self):
        return self._hop

    def win_length(self):
        return self._wl

    def bins(self):
        return self._n // 2 + 1

    def frames(self, length):
        """Frames of a row of `length` reals; 0 where the length is invalid."""
        return int(self._fn("frames")(self._h, int(length)))

    def default_length(self, frames):
        """The longest row `frames` frames give back: hop * (frames - 1) + n_fft - 2 * padding."""
        return self._hop * (int(frames) - 1) + self._n - 2 * self._pad

    def set_option(self, key, value):
        """"fusion": 0 = the composed forward route, 1 = the fused one-launch route wherever it exists."""
        self._call("set_option", key.encode(), int(value), message=f"bad option {key}={value}")

    def reserve(self, length, batch):
        """Later forward calls of at most `batch` rows of `length` reals, and inverse calls to that length from frames(length) frames,
        never allocate."""
        self._call("reserve", int(length), int(batch))

    def set_window_ptr(self, d_window, stream=0):
        """win_length() reals of the handle's precision at d_window (0 / None: all ones).  Waits for `stream`."""
        self._call("set_window", d_window or None, stream)

    def forward_ptr(self, d_in, d_out, length, batch, normalized=False, stream=0):
        """`batch` rows of `length` reals at d_in -> batch x frames(length) x bins() complex at d_out, enqueued on `stream`."""
        self._call("forward", d_in, d_out, int(length), int(batch), int(bool(normalized)), stream)

    def inverse_ptr(self, d_in, d_out, frames, length, batch, normalized=False, stream=0):
        """batch x frames x bins() complex at d_in -> `batch` rows of `length` reals at d_out, enqueued on `stream`."""
        self._call("inverse", d_in, d_out, int(frames), int(length), int(batch), int(bool(normalized)), stream)

    def set_window(self, window):
        """A contiguous CUDA tensor of win_length() reals of the handle's precision, or None for all ones; on the current stream."""
        if window is None:
            return self.set_window_ptr(None)
        _require_cuda(window, _torch_dtypes(self.real)[0])
        if tuple(window.shape) != (self._wl,):
            raise ValueError(f"window must have shape ({self._wl},), got {tuple(window.shape)}")
        self.set_window_ptr(window.data_ptr(), _stream(window))

    def forward(self, x, normalized=False, out=None):
        """Contiguous (..., length) real CUDA tensor -> a new (..., frames, bins) complex tensor (frame-major), or `out`, on the current
        stream."""
        import torch

        rdt, cdt = _torch_dtypes(self.real)
        _require_cuda(x, rdt)
        if x.dim() == 0:
            raise ValueError("expected at least one dimension")
        length = int(x.shape[-1])
        fr = self.frames(length)
        if fr == 0:
            raise ValueError(f"a row of {length} samples is too short for n_fft {self._n} with padding {self.pad_mode}")
        shape = tuple(x.shape[:-1]) + (fr, self.bins())
        if out is None:
            out = torch.empty(shape, dtype=cdt, device=x.device)
        else:
            _require_out(out, shape, cdt, x.device)
        batch = x.numel() // length
        if batch:
            self.forward_ptr(x.data_ptr(), out.data_ptr(), length, batch, normalized, _stream(x))
        return out

    def inverse(self, X, length=None, normalized=False, out=None):
        """Contiguous (..., frames, bins) complex CUDA tensor (frame-major) -> a new (..., length) real tensor, or `out`, on the current
        stream; length defaults to default_length(frames)."""
        import torch

        rdt, cdt = _torch_dtypes(self.real)
        _require_cuda(X, cdt)
        if X.dim() < 2 or X.shape[-1] != self.bins() or X.shape[-2] == 0:
            raise ValueError(f"expected (..., frames >= 1, {self.bins()}), got {tuple(X.shape)}")
        fr = int(X.shape[-2])
        full = self.default_length(fr)
        length = full if length is None else int(length)
        if not 1 <= length <= full:
            raise ValueError(f"length must be in 1 ... {full} for {fr} frames, got {length}")
        shape = tuple(X.shape[:-2]) + (length,)
        if out is None:
            out = torch.empty(shape, dtype=rdt, device=X.device)
        else:
            _require_out(out, shape, rdt, X.device)
        batch = X.numel() // (fr * self.bins())
        self.inverse_ptr(X.data_ptr(), out.data_ptr(), fr, length, batch, normalized, _stream(X))
        return out


def create_stft_f32(n_fft, hop_length=None, win_length=None, center=True, pad_mode="reflect", device=-1):
    return Stft(n_fft, "f32", hop_length, win_length, center, pad_mode, device)


def create_stft_f64(n_fft, hop_length=None, win_length=None, center=True, pad_mode="reflect", device=-1):
    return Stft(n_fft, "f64", hop_length, win_length, center, pad_mode, device)


def _stft_plan(x, n_fft, hop_length, win_length, window, center, pad_mode, real, cls=None):
    """The cached handle of these parameters with `window` set (on every call, like fftconv's filters)."""
    n_fft = int(n_fft)
    hop = n_fft // 4 if hop_length is None else int(hop_length)
    wl = n_fft if win_length is None else int(win_length)
    mode = _stft_pad_mode(center, pad_mode)
    if n_fft < 1 or hop < 1 or not 1 <= wl <= n_fft:
        raise ValueError(f"need n_fft >= 1, hop_length >= 1 and 1 <= win_length <= n_fft, got {n_fft}, {hop}, {wl}")
    if window is not None:
        if not (_is_torch(window) and window.is_cuda and window.dtype == _torch_dtypes(real)[0] and window.device == x.device):
            raise TypeError(f"window must be a CUDA {_names((_torch_dtypes(real)[0],))} tensor on the input's device")
        if tuple(window.shape) != (wl,):
            raise ValueError(f"window must have shape ({wl},), got {tuple(window.shape)}")
        window = window.contiguous()
    p = _cached_plan(cls or Stft, n_fft, real, hop, wl, mode != "none", "reflect" if mode == "none" else mode, int(_device_index(x)))
    p.set_window(window)
    return p


def stft(x, n_fft, hop_length=None, win_length=None, window=None, center=True, pad_mode="reflect", normalized=False):
    """torch.stft(..., onesided=True, return_complex=True) of a float32 / float64 CUDA tensor of shape (..., length) on the current
    stream, torch's defaults (hop_length n_fft // 4, win_length n_fft, window of ones); pad_mode "reflect" or "constant".  Returns shape
    (..., bins, frames) like torch -- the TRANSPOSED VIEW of the frame-major buffer the library writes (bins contiguous per frame), not
    a contiguous tensor; istft takes it back without a copy.  Leading dimensions fold into the batch.  Handles are cached per
    (n_fft, hop, win_length, padding, dtype, device) and the window is set on EVERY call; keep an Stft to reuse one."""
    import torch

    if not (_is_torch(x) and x.is_cuda and x.dtype in (torch.float32, torch.float64)):
        raise TypeError("expected a CUDA float32 / float64 tensor")
    if x.dim() == 0:
        raise ValueError("expected at least one dimension")
    p = _stft_plan(x, n_fft, hop_length, win_length, window, center, pad_mode, _precision(x.dtype)[0])
    return p.forward(x.contiguous(), normalized).transpose(-1, -2)


def istft(X, n_fft, hop_length=None, win_length=None, window=None, center=True, normalized=False, length=None):
    """torch.istft(..., onesided=True) of a complex64 / complex128 CUDA tensor of shape (..., bins, frames) on the current stream ->
    (..., length) reals, length defaulting to hop * (frames - 1) + n_fft - 2 * padding.  A tensor that is the transposed view stft
    returns is used as it is; any other layout is copied into frame-major order first.  A window whose overlap-add envelope falls
    below 1e-11 on a kept sample raises FourierError (torch's NOLA check)."""
    import torch

    if not (_is_torch(X) and X.is_cuda and X.dtype in (torch.complex64, torch.complex128)):
        raise TypeError("expected a CUDA complex64 / complex128 tensor")
    if X.dim() < 2:
        raise ValueError("expected shape (..., bins, frames)")
    if X.shape[-2] != int(n_fft) // 2 + 1 or X.shape[-1] == 0:
        raise ValueError(f"expected (..., {int(n_fft) // 2 + 1}, frames >= 1), got {tuple(X.shape)}")
    p = _stft_plan(X, n_fft, hop_length, win_length, window, center, "reflect", _precision(X.dtype)[0])
    return p.inverse(X.transpose(-1, -2).contiguous(), length, normalized)


SPECTROGRAM_POWERS = {"magnitude": 1, "power": 2}  # FOURIER_SPECTROGRAM_MAGNITUDE / _POWER


def _spectrogram_power(power):
    if power in (1, 2):  # (1.0 and 2.0 compare equal: torchaudio's power is a float)
        return int(power)
    raise ValueError(f"power must be 1 (magnitude) or 2 (power), got {power!r}")


class Spectrogram(_Handle):
    """Batched power spectrogram and Welch average (include/fourier.h, fourier_hip_spectrogram_*) on device memory: |X|^p of the frames X
    an Stft of the same parameters gives, FRAME-MAJOR reals (frame f of row b at element offset (b * frames + f) * bins), and the mean
    over the frames of |X|^2 -- neither writes the complex frames.  n_fft, hop, win_length and the padding are fixed at create; the
    window is set afterwards (set_window; default all ones)."""

    _prefix = "fourier_hip_spectrogram_"
    _destroy = "fourier_hip_spectrogram_destroy"

    def __init__(self, n_fft, real="f32", hop_length=None, win_length=None, center=True, pad_mode="reflect", device=-1):
        n_fft = int(n_fft)
        hop = n_fft // 4 if hop_length is None else int(hop_length)
        wl = n_fft if win_length is None else int(win_length)
        self.pad_mode = _stft_pad_mode(center, pad_mode)
        if n_fft < 1 or hop < 1 or not 1 <= wl <= n_fft:
            raise ValueError(f"need n_fft >= 1, hop_length >= 1 and 1 <= win_length <= n_fft, got {n_fft}, {hop}, {wl}")
        self._create(real, f"spectrogram plan of n_fft {n_fft}, hop {hop}, win_length {wl}, padding {self.pad_mode}", n_fft, hop, wl,
                     STFT_PAD_MODES[self.pad_mode], int(device))
        self._n, self._hop, self._wl = n_fft, hop, wl

    def n_fft(self):
        return self._n

    def hop(self):
        return self._hop

    def win_length(self):
        return self._wl

    def bins(self):
        return self._n // 2 + 1

    def frames(self, length):
        """Frames of a row of `length` reals; 0 where the length is invalid."""
        return int(self._fn("frames")(self._h, int(length)))

    def set_option(self, key, value):
        """"fusion": 0 = the composed routes (the default), 1 = the fused one-launch routes wherever they exist."""
        self._call("set_option", key.encode(), int(value), message=f"bad option {key}={value}")

    def reserve(self, length, batch):
        """Later forward and welch calls of at most `batch` rows of `length` reals never allocate (on the route selected now)."""
        self._call("reserve", int(length), int(batch))

    def set_window_ptr(self, d_window, stream=0):
        """win_length() reals of the handle's precision at d_window (0 / None: all ones).  Waits for `stream`."""
        self._call("set_window", d_window or None, stream)

    def forward_ptr(self, d_in, d_out, length, batch, power=2, normalized=False, stream=0):
        """`batch` rows of `length` reals at d_in -> batch x frames(length) x bins() reals |X|^power at d_out, enqueued on `stream`."""
        self._call("forward", d_in, d_out, int(length), int(batch), int(power), int(bool(normalized)), stream)

    def welch_ptr(self, d_in, d_out, length, batch, onesided_fold=True, scale=1.0, stream=0):
        """`batch` rows of `length` reals at d_in -> batch x bins() reals scale * c_k / frames * sum_f |X|^2 at d_out, on `stream`."""
        self._call("welch", d_in, d_out, int(length), int(batch), int(bool(onesided_fold)), float(scale), stream)

    def set_window(self, window):
        """A contiguous CUDA tensor of win_length() reals of the handle's precision, or None for all ones; on the current stream."""
        if window is None:
            return self.set_window_ptr(None)
        _require_cuda(window, _torch_dtypes(self.real)[0])
        if tuple(window.shape) != (self._wl,):
            raise ValueError(f"window must have shape ({self._wl},), got {tuple(window.shape)}")
        self.set_window_ptr(window.data_ptr(), _stream(window))

    def _rows(self, x):
        rdt = _torch_dtypes(self.real)[0]
        _require_cuda(x, rdt)
        if x.dim() == 0:
            raise ValueError("expected at least one dimension")
        length = int(x.shape[-1])
        fr = self.frames(length)
        if fr == 0:
            raise ValueError(f"a row of {length} samples is too short for n_fft {self._n} with padding {self.pad_mode}")
        return rdt, length, fr

    def forward(self, x, power=2, normalized=False, out=None):
        """Contiguous (..., length) real CUDA tensor -> a new (..., frames, bins) real tensor |X|^power (frame-major), or `out`, on the
        current stream."""
        import torch

        power = _spectrogram_power(power)
        rdt, length, fr = self._rows(x)
        shape = tuple(x.shape[:-1]) + (fr, self.bins())
        if out is None:
            out = torch.empty(shape, dtype=rdt, device=x.device)
        else:
            _require_out(out, shape, rdt, x.device)
        batch = x.numel() // length
        if batch:
            self.forward_ptr(x.data_ptr(), out.data_ptr(), length, batch, power, normalized, _stream(x))
        return out

    def welch(self, x, onesided_fold=True, scale=1.0, out=None):
        """Contiguous (..., length) real CUDA tensor -> a new (..., bins) real tensor scale * c_k / frames * sum_f |X|^2, or `out`, on
        the current stream.  No detrending."""
        import torch

        rdt, length, fr = self._rows(x)
        shape = tuple(x.shape[:-1]) + (self.bins(),)
        if out is None:
            out = torch.empty(shape, dtype=rdt, device=x.device)
        else:
            _require_out(out, shape, rdt, x.device)
        batch = x.numel() // length
        if batch:
            self.welch_ptr(x.data_ptr(), out.data_ptr(), length, batch, onesided_fold, scale, _stream(x))
        return out


def create_spectrogram_f32(n_fft, hop_length=None, win_length=None, center=True, pad_mode="reflect", device=-1):
    return Spectrogram(n_fft, "f32", hop_length, win_length, center, pad_mode, device)


def create_spectrogram_f64(n_fft, hop_length=None, win_length=None, center=True, pad_mode="reflect", device=-1):
    return Spectrogram(n_fft, "f64", hop_length, win_length, center, pad_mode, device)


def _real_rows(x):
    import torch

    if not (_is_torch(x) and x.is_cuda and x.dtype in (torch.float32, torch.float64)):
        raise TypeError("expected a CUDA float32 / float64 tensor")
    if x.dim() == 0:
        raise ValueError("expected at least one dimension")
    return _precision(x.dtype)[0]


def spectrogram(x, n_fft, hop_length=None, win_length=None, window=None, center=True, pad_mode="reflect", power=2.0, normalized=False):
    """torchaudio.transforms.Spectrogram of a float32 / float64 CUDA tensor of shape (..., length) on the current stream: |stft|^power
    with power 1 or 2, torch.stft's defaults (hop_length n_fft // 4, win_length n_fft, window of ones) and `normalized` as torch.stft's
    flag (the frames times n_fft^-1/2).  Returns shape (..., frames, bins), FRAME-MAJOR and contiguous like the buffer the library
    writes -- torchaudio's (..., bins, frames) is its transpose(-1, -2).  Leading dimensions fold into the batch.  Handles are cached
    per (n_fft, hop, win_length, padding, dtype, device) and the window is set on EVERY call; keep a Spectrogram to reuse one."""
    real = _real_rows(x)
    power = _spectrogram_power(power)
    p = _stft_plan(x, n_fft, hop_length, win_length, window, center, pad_mode, real, Spectrogram)
    return p.forward(x.contiguous(), power, normalized)


WELCH_SCALINGS = ("density", "spectrum")


def welch(x, fs=1.0, window=None, nperseg=256, noverlap=None, scaling="density", return_onesided=True):
    """scipy.signal.welch(x, fs, window, nperseg, noverlap, detrend=False, scaling=scaling, average="mean") along the last axis of a
    float32 / float64 CUDA tensor of shape (..., length) on the current stream.  Segments of nperseg samples every nperseg - noverlap
    (noverlap defaults to nperseg // 2), no padding, the periodic Hann window where `window` is None, else a CUDA tensor of nperseg
    values.  scaling "density" gives V^2 / Hz (scale 1 / (fs sum w^2)), "spectrum" V^2 (1 / (sum w)^2), both computed on the host in
    f64 from the window.  Returns (freqs, Pxx): nperseg // 2 + 1 frequencies k fs / nperseg and (..., nperseg // 2 + 1) values; with
    return_onesided the bins that have a mirror count twice, without it they do not (the one-sided HALF of the two-sided spectrum).
    NO DETRENDING: scipy's default, detrend="constant", removes every segment's mean first; this never does, and offers no `detrend`
    argument.  Subtract the mean yourself where the difference at the lowest bins matters."""
    p, scale, freqs = _welch_plan(x, fs, window, nperseg, noverlap, scaling, Spectrogram)
    return freqs, p.welch(x.contiguous(), bool(return_onesided), scale)


class CrossSpectrum(_Handle):
    """Batched cross-spectral density and coherence of two signals (include/fourier.h, fourier_hip_csd_*) on device memory: of the frames
    X and Y an Stft of the same parameters gives for a row of x and the same row of y, scale * c_k / frames * sum_f conj(X) Y (complex)
    and |sum_f conj(X) Y|^2 / (sum_f |X|^2 sum_f |Y|^2) (real) -- neither writes a frame.  n_fft, hop, win_length and the padding are
    fixed at create; the window is set afterwards (set_window; default all ones)."""

    _prefix = "fourier_hip_csd_"
    _destroy = "fourier_hip_csd_destroy"

    def __init__(self, n_fft, real="f32", hop_length=None, win_length=None, center=True, pad_mode="reflect", device=-1):
        n_fft = int(n_fft)
        hop = n_fft // 4 if hop_length is None else int(hop_length)
        wl = n_fft if win_length is None else int(win_length)
        self.pad_mode = _stft_pad_mode(center, pad_mode)
        if n_fft < 1 or hop < 1 or not 1 <= wl <= n_fft:
            raise ValueError(f"need n_fft >= 1, hop_length >= 1 and 1 <= win_length <= n_fft, got {n_fft}, {hop}, {wl}")
        self._create(real, f"cross-spectrum plan of n_fft {n_fft}, hop {hop}, win_length {wl}, padding {self.pad_mode}", n_fft, hop, wl,
                     STFT_PAD_MODES[self.pad_mode], int(device))
        self._n, self._hop, self._wl = n_fft, hop, wl

    # the framing, the window and the options are the spectrogram handle's
    n_fft, hop, win_length, bins, frames = Spectrogram.n_fft, Spectrogram.hop, Spectrogram.win_length, Spectrogram.bins, Spectrogram.frames
    set_option, set_window_ptr, set_window, _rows = Spectrogram.set_option, Spectrogram.set_window_ptr, Spectrogram.set_window, Spectrogram._rows

    def reserve(self, length, batch):
        """Later csd and coherence calls of at most `batch` rows of `length` reals never allocate (on the route selected now)."""
        self._call("reserve", int(length), int(batch))

    def csd_ptr(self, d_x, d_y, d_out, length, batch, onesided_fold=True, scale=1.0, stream=0):
        """`batch` rows of `length` reals at d_x and at d_y -> batch x bins() complex values scale * c_k / frames * sum_f conj(X) Y at
        d_out, enqueued on `stream`."""
        self._call("csd", d_x, d_y, d_out, int(length), int(batch), int(bool(onesided_fold)), float(scale), stream)

    def coherence_ptr(self, d_x, d_y, d_out, length, batch, stream=0):
        """... -> batch x bins() reals |sum_f conj(X) Y|^2 / (sum_f |X|^2 sum_f |Y|^2) at d_out, on `stream`."""
        self._call("coherence", d_x, d_y, d_out, int(length), int(batch), stream)

    def _pair(self, x, y, out, out_dtype):
        import torch

        rdt, length, _ = self._rows(x)
        _require_cuda(y, rdt)
        if tuple(y.shape) != tuple(x.shape) or y.device != x.device:
            raise ValueError(f"x and y must have the same shape and device, got {tuple(x.shape)} and {tuple(y.shape)}")
        shape = tuple(x.shape[:-1]) + (self.bins(),)
        if out is None:
            out = torch.empty(shape, dtype=out_dtype, device=x.device)
        else:
            _require_out(out, shape, out_dtype, x.device)
        return out, length, x.numel() // length

    def csd(self, x, y, onesided_fold=True, scale=1.0, out=None):
        """Contiguous (..., length) real CUDA tensors x and y of one shape -> a new (..., bins) complex tensor
        scale * c_k / frames * sum_f conj(X) Y, or `out`, on the current stream.  No detrending."""
        out, length, batch = self._pair(x, y, out, _torch_dtypes(self.real)[1])
        if batch:
            self.csd_ptr(x.data_ptr(), y.data_ptr(), out.data_ptr(), length, batch, onesided_fold, scale, _stream(x))
        return out

    def coherence(self, x, y, out=None):
        """... -> a new (..., bins) real tensor |sum_f conj(X) Y|^2 / (sum_f |X|^2 sum_f |Y|^2), or `out`.  No detrending."""
        out, length, batch = self._pair(x, y, out, _torch_dtypes(self.real)[0])
        if batch:
            self.coherence_ptr(x.data_ptr(), y.data_ptr(), out.data_ptr(), length, batch, _stream(x))
        return out


def create_csd_f32(n_fft, hop_length=None, win_length=None, center=True, pad_mode="reflect", device=-1):
    return CrossSpectrum(n_fft, "f32", hop_length, win_length, center, pad_mode, device)


def create_csd_f64(n_fft, hop_length=None, win_length=None, center=True, pad_mode="reflect", device=-1):
    return CrossSpectrum(n_fft, "f64", hop_length, win_length, center, pad_mode, device)


def _welch_plan(x, fs, window, nperseg, noverlap, scaling, cls):
    """welch's argument rules: the cached handle of class `cls` with the window set, the scale of `scaling` and the frequencies"""
    import torch

    real = _real_rows(x)
    nperseg = int(nperseg)
    noverlap = nperseg // 2 if noverlap is None else int(noverlap)
    if nperseg < 1 or not 0 <= noverlap < nperseg:
        raise ValueError(f"need nperseg >= 1 and 0 <= noverlap < nperseg, got {nperseg}, {noverlap}")
    if scaling not in WELCH_SCALINGS:
        raise ValueError(f"scaling must be 'density' or 'spectrum', got {scaling!r}")
    if not float(fs) > 0:
        raise ValueError(f"fs must be positive, got {fs!r}")
    if x.shape[-1] < nperseg:
        raise ValueError(f"a row of {x.shape[-1]} samples is shorter than nperseg {nperseg}")
    if window is None:
        window = torch.hann_window(nperseg, periodic=True, dtype=torch.float64, device=x.device).to(x.dtype)
    p = _stft_plan(x, nperseg, nperseg - noverlap, nperseg, window, False, "reflect", real, cls)
    w = window.detach().to(torch.float64).cpu()
    scale = 1.0 / (float(fs) * float((w * w).sum())) if scaling == "density" else 1.0 / float(w.sum()) ** 2
    freqs = torch.arange(nperseg // 2 + 1, dtype=x.dtype, device=x.device) * (float(fs) / nperseg)
    return p, scale, freqs


def _same_rows(x, y):
    _real_rows(x)
    if not (_is_torch(y) and y.is_cuda and y.dtype == x.dtype):
        raise TypeError(f"y must be a CUDA {_names((x.dtype,))} tensor like x")
    if tuple(y.shape) != tuple(x.shape) or y.device != x.device:
        raise ValueError(f"x and y must have the same shape and device, got {tuple(x.shape)} and {tuple(y.shape)}")


def csd(x, y, fs=1.0, window=None, nperseg=256, noverlap=None, scaling="density", return_onesided=True):
    """scipy.signal.csd(x, y, fs, window, nperseg, noverlap, detrend=False, scaling=scaling, average="mean") along the last axis of two
    float32 / float64 CUDA tensors of one shape (..., length) on the current stream.  Segments, window default, scaling and
    return_onesided are welch's: segments of nperseg samples every nperseg - noverlap (noverlap defaults to nperseg // 2), no padding,
    the periodic Hann window where `window` is None.  Returns (freqs, Pxy): nperseg // 2 + 1 frequencies k fs / nperseg and
    (..., nperseg // 2 + 1) complex values, the mean over the segments of conj(X) Y times the scale.
    NO DETRENDING: scipy's default, detrend="constant", removes every segment's mean first; this never does, and offers no `detrend`
    argument.  Subtract the mean yourself where the difference at the lowest bins matters."""
    _same_rows(x, y)
    p, scale, freqs = _welch_plan(x, fs, window, nperseg, noverlap, scaling, CrossSpectrum)
    return freqs, p.csd(x.contiguous(), y.contiguous(), bool(return_onesided), scale)


def coherence(x, y, fs=1.0, window=None, nperseg=256, noverlap=None):
    """scipy.signal.coherence(x, y, fs, window, nperseg, noverlap, detrend=False): |Pxy|^2 / (Pxx Pyy) of welch's segments along the last
    axis of two float32 / float64 CUDA tensors of one shape (..., length) on the current stream.  Returns (freqs, Cxy) with
    (..., nperseg // 2 + 1) reals; a bin whose denominator is 0 gives what the IEEE division gives.
    NO DETRENDING: scipy's default, detrend="constant", removes every segment's mean first; this never does, and offers no `detrend`
    argument.  Subtract the mean yourself where the difference at the lowest bins matters."""
    _same_rows(x, y)
    p, _, freqs = _welch_plan(x, fs, window, nperseg, noverlap, "density", CrossSpectrum)
    return freqs, p.coherence(x.contiguous(), y.contiguous())


class BandSpectrogram(_Handle):
    """Batched band-energy spectrogram (include/fourier.h, fourier_hip_bandspec_*) on device memory: the |X|^p of the frames X an Stft of
    the same parameters gives, projected onto the rows of a real `bands` x bins matrix W -- a mel bank (mel_filterbank), or any matrix
    whose rows have short supports; negative weights are allowed -- Y[b, f, j] = sum_k W[j, k] |X[b, f, k]|^p, optionally
    log_mult * ln(max(Y, log_floor)), FRAME-MAJOR reals (frame f of row b at element offset (b * frames + f) * bands).  |X|^p is never
    written anywhere the caller sees.  n_fft, hop, win_length, the padding and the number of bands are fixed at create; the window
    (set_window; default all ones) and the bank (set_bands; forward raises without one) are set afterwards."""

    _prefix = "fourier_hip_bandspec_"
    _destroy = "fourier_hip_bandspec_destroy"

    def __init__(self, n_fft, bands, real="f32", hop_length=None, win_length=None, center=True, pad_mode="reflect", device=-1):
        n_fft, bands = int(n_fft), int(bands)
        hop = n_fft // 4 if hop_length is None else int(hop_length)
        wl = n_fft if win_length is None else int(win_length)
        self.pad_mode = _stft_pad_mode(center, pad_mode)
        if n_fft < 1 or hop < 1 or not 1 <= wl <= n_fft:
            raise ValueError(f"need n_fft >= 1, hop_length >= 1 and 1 <= win_length <= n_fft, got {n_fft}, {hop}, {wl}")
        if not 1 <= bands <= 65535:
            raise ValueError(f"need 1 <= bands <= 65535, got {bands}")
        self._create(real, f"band-spectrogram plan of n_fft {n_fft}, hop {hop}, win_length {wl}, padding {self.pad_mode}, {bands} bands",
                     n_fft, hop, wl, STFT_PAD_MODES[self.pad_mode], bands, int(device))
        self._n, self._hop, self._wl, self._bands = n_fft, hop, wl, bands

    # the framing, the window and the options are the spectrogram handle's
    n_fft, hop, win_length, bins, frames = Spectrogram.n_fft, Spectrogram.hop, Spectrogram.win_length, Spectrogram.bins, Spectrogram.frames
    set_window_ptr, set_window, _rows = Spectrogram.set_window_ptr, Spectrogram.set_window, Spectrogram._rows

    def bands(self):
        return self._bands

    def set_option(self, key, value):
        """"fusion": 0 = the composed route, 1 = the fused one-launch route wherever it exists (bands <= bins; the default there)."""
        self._call("set_option", key.encode(), int(value), message=f"bad option {key}={value}")

    def reserve(self, length, batch):
        """Later forward calls of at most `batch` rows of `length` reals never allocate (on the route selected now)."""
        self._call("reserve", int(length), int(batch))

    def set_bands_ptr(self, h_matrix, stream=0):
        """bands() x bins() reals of the handle's precision, row-major, at the HOST address h_matrix.  Waits for `stream`."""
        self._call("set_bands", h_matrix, stream)

    def set_bands(self, matrix):
        """A numpy array or a torch tensor (any device) of shape (bands, bins): moved to the host and cast to the handle's precision.
        Every weight must be finite.  Replaces the bank in use; waits for the current stream."""
        import numpy as np

        if _is_torch(matrix):
            matrix = matrix.detach().cpu().numpy()
        elif not isinstance(matrix, np.ndarray):
            raise TypeError("matrix must be a numpy array or a torch tensor")
        if matrix.dtype.kind not in "fiu":
            raise TypeError(f"matrix must be real, got {matrix.dtype}")
        if tuple(matrix.shape) != (self._bands, self.bins()):
            raise ValueError(f"matrix must have shape ({self._bands}, {self.bins()}), got {tuple(matrix.shape)}")
        host = np.ascontiguousarray(matrix, dtype=np.float32 if self.real == "f32" else np.float64)
        if not np.isfinite(host).all():
            raise ValueError("every band weight must be finite")
        stream = 0
        try:
            import torch

            if torch.cuda.is_available():
                stream = torch.cuda.current_stream().cuda_stream
        except Exception:
            pass
        self.set_bands_ptr(host.ctypes.data, stream)

    def forward_ptr(self, d_in, d_out, length, batch, power=2, normalized=False, log_mult=0.0, log_floor=0.0, stream=0):
        """`batch` rows of `length` reals at d_in -> batch x frames(length) x bands() reals at d_out, enqueued on `stream`."""
        self._call("forward", d_in, d_out, int(length), int(batch), int(power), int(bool(normalized)), float(log_mult), float(log_floor), stream)

    def forward(self, x, power=2, normalized=False, log_mult=0.0, log_floor=0.0, out=None):
        """Contiguous (..., length) real CUDA tensor -> a new (..., frames, bands) real tensor (frame-major), or `out`, on the current
        stream.  log_mult 0: the band energies; else log_mult * ln(max(energy, log_floor)) with log_floor > 0."""
        import math

        import torch

        power = _spectrogram_power(power)
        log_mult, log_floor = float(log_mult), float(log_floor)
        if not math.isfinite(log_mult):
            raise ValueError(f"log_mult must be finite, got {log_mult}")
        if log_mult != 0.0 and not (math.isfinite(log_floor) and log_floor > 0.0):
            raise ValueError(f"log_floor must be finite and > 0 when log_mult != 0, got {log_floor}")
        rdt, length, fr = self._rows(x)
        shape = tuple(x.shape[:-1]) + (fr, self._bands)
        if out is None:
            out = torch.empty(shape, dtype=rdt, device=x.device)
        else:
            _require_out(out, shape, rdt, x.device)
        batch = x.numel() // length
        if batch:
            self.forward_ptr(x.data_ptr(), out.data_ptr(), length, batch, power, normalized, log_mult, log_floor, _stream(x))
        return out


def create_bandspec_f32(n_fft, bands, hop_length=None, win_length=None, center=True, pad_mode="reflect", device=-1):
    return BandSpectrogram(n_fft, bands, "f32", hop_length, win_length, center, pad_mode, device)


def create_bandspec_f64(n_fft, bands, hop_length=None, win_length=None, center=True, pad_mode="reflect", device=-1):
    return BandSpectrogram(n_fft, bands, "f64", hop_length, win_length, center, pad_mode, device)


MEL_SCALES = ("htk", "slaney")
MEL_LOGS = (None, "ln", "log10", "db")


def _hz_to_mel(f, mel_scale):
    import numpy as np

    f = np.asarray(f, dtype=np.float64)
    if mel_scale == "htk":
        return 2595.0 * np.log10(1.0 + f / 700.0)
    lin = f / (200.0 / 3.0)
    return np.where(f >= 1000.0, 15.0 + np.log(np.maximum(f, 1000.0) / 1000.0) / (np.log(6.4) / 27.0), lin)


def _mel_to_hz(m, mel_scale):
    import numpy as np

    m = np.asarray(m, dtype=np.float64)
    if mel_scale == "htk":
        return 700.0 * (10.0 ** (m / 2595.0) - 1.0)
    return np.where(m >= 15.0, 1000.0 * np.exp((np.log(6.4) / 27.0) * (m - 15.0)), (200.0 / 3.0) * m)


def mel_filterbank(n_freqs, f_min, f_max, n_mels, sample_rate, norm=None, mel_scale="htk"):
    """The triangular mel bank as a numpy float64 (n_mels, n_freqs) matrix: the transpose of
    torchaudio.functional.melscale_fbanks(n_freqs, f_min, f_max, n_mels, sample_rate, norm, mel_scale).  Column k stands for the
    frequency k * (sample_rate / 2) / (n_freqs - 1); n_mels + 2 points equally spaced in mel between f_min and f_max give the corners
    f_pts of the triangles, W[j, k] = max(0, min((f_k - f_pts[j]) / (f_pts[j+1] - f_pts[j]), (f_pts[j+2] - f_k) / (f_pts[j+2] - f_pts[j+1]))).
    norm "slaney" scales row j by 2 / (f_pts[j+2] - f_pts[j]) (unit area); mel_scale "htk": mel = 2595 log10(1 + f / 700), "slaney":
    f / (200 / 3) below 1000 Hz and 15 + ln(f / 1000) / (ln(6.4) / 27) from there on."""
    import numpy as np

    n_freqs, n_mels = int(n_freqs), int(n_mels)
    f_min, f_max, sample_rate = float(f_min), float(f_max), float(sample_rate)
    if norm not in (None, "slaney"):
        raise ValueError(f"norm must be None or 'slaney', got {norm!r}")
    if mel_scale not in MEL_SCALES:
        raise ValueError(f"mel_scale must be 'htk' or 'slaney', got {mel_scale!r}")
    if n_freqs < 2 or n_mels < 1:
        raise ValueError(f"need n_freqs >= 2 and n_mels >= 1, got {n_freqs}, {n_mels}")
    if not (sample_rate > 0 and 0 <= f_min < f_max):
        raise ValueError(f"need sample_rate > 0 and 0 <= f_min < f_max, got {sample_rate}, {f_min}, {f_max}")
    all_freqs = np.linspace(0.0, sample_rate / 2.0, n_freqs)
    m_pts = np.linspace(float(_hz_to_mel(f_min, mel_scale)), float(_hz_to_mel(f_max, mel_scale)), n_mels + 2)
    f_pts = _mel_to_hz(m_pts, mel_scale)
    f_diff = f_pts[1:] - f_pts[:-1]
    slopes = f_pts[:, None] - all_freqs[None, :]  # (n_mels + 2, n_freqs)
    up = -slopes[:-2] / f_diff[:-1, None]
    down = slopes[2:] / f_diff[1:, None]
    W = np.maximum(0.0, np.minimum(up, down))
    if norm == "slaney":
        W *= (2.0 / (f_pts[2:] - f_pts[:-2]))[:, None]
    return W


def _bandspec_plan(x, matrix, n_fft, hop_length, win_length, window, center, pad_mode, real):
    """The cached handle of these parameters with `window` and the bank set (on every call, like fftconv's filters)."""
    import numpy as np

    if not (_is_torch(matrix) or isinstance(matrix, np.ndarray)):
        raise TypeError("matrix must be a numpy array or a torch tensor")
    if matrix.ndim != 2 or matrix.shape[1] != int(n_fft) // 2 + 1 or matrix.shape[0] < 1:
        raise ValueError(f"matrix must have shape (bands >= 1, {int(n_fft) // 2 + 1}), got {tuple(matrix.shape)}")
    bands = int(matrix.shape[0])
    n_fft = int(n_fft)
    hop = n_fft // 4 if hop_length is None else int(hop_length)
    wl = n_fft if win_length is None else int(win_length)
    mode = _stft_pad_mode(center, pad_mode)
    if n_fft < 1 or hop < 1 or not 1 <= wl <= n_fft:
        raise ValueError(f"need n_fft >= 1, hop_length >= 1 and 1 <= win_length <= n_fft, got {n_fft}, {hop}, {wl}")
    if window is not None:
        if not (_is_torch(window) and window.is_cuda and window.dtype == _torch_dtypes(real)[0] and window.device == x.device):
            raise TypeError(f"window must be a CUDA {_names((_torch_dtypes(real)[0],))} tensor on the input's device")
        if tuple(window.shape) != (wl,):
            raise ValueError(f"window must have shape ({wl},), got {tuple(window.shape)}")
        window = window.contiguous()
    p = _cached_plan(BandSpectrogram, n_fft, bands, real, hop, wl, mode != "none", "reflect" if mode == "none" else mode, int(_device_index(x)))
    p.set_window(window)
    p.set_bands(matrix)
    return p


def band_spectrogram(x, matrix, n_fft, hop_length=None, win_length=None, window=None, center=True, pad_mode="reflect", power=2.0,
                     normalized=False, log_mult=0.0, log_floor=0.0):
    """spectrogram(x, ...) projected onto the rows of `matrix`, a numpy array or torch tensor of shape (bands, n_fft // 2 + 1), without
    the spectrogram being written: a float32 / float64 CUDA tensor of shape (..., length) -> (..., frames, bands), FRAME-MAJOR and
    contiguous, on the current stream; log_mult != 0 gives log_mult * ln(max(., log_floor)).  Leading dimensions fold into the batch.
    Handles are cached per (n_fft, bands, hop, win_length, padding, dtype, device); the window and the bank are set on EVERY call, and
    setting a bank waits for the stream -- keep a BandSpectrogram to reuse one."""
    real = _real_rows(x)
    power = _spectrogram_power(power)
    p = _bandspec_plan(x, matrix, n_fft, hop_length, win_length, window, center, pad_mode, real)
    return p.forward(x.contiguous(), power, normalized, log_mult, log_floor)


def mel_spectrogram(x, sample_rate, n_fft, n_mels=128, f_min=0.0, f_max=None, hop_length=None, win_length=None, window=None, center=True,
                    pad_mode="reflect", power=2.0, normalized=False, norm=None, mel_scale="htk", log=None, amin=1e-10, ref=1.0, top_db=None):
    """torchaudio.transforms.MelSpectrogram of a float32 / float64 CUDA tensor of shape (..., length) on the current stream, with the
    defaults of spectrogram() (hop_length n_fft // 4, window of ones) -> (..., frames, n_mels), FRAME-MAJOR (torchaudio's
    (..., n_mels, frames) is its transpose(-1, -2)).  f_max defaults to sample_rate / 2.  log: None = the mel energies Y; "ln" =
    ln(max(Y, amin)); "log10" = log10(max(Y, amin)); "db" = (10 if power == 2 else 20) * log10(max(Y, amin) / ref), librosa's
    power_to_db / amplitude_to_db with a scalar ref.  The logarithm of the floored value runs in the kernel; the `ref` offset and the
    `top_db` clamp ("db" only: nothing below the maximum of each leading item's (frames, n_mels) block minus top_db) are torch
    operations on the small output."""
    import math

    real = _real_rows(x)
    power = _spectrogram_power(power)
    if log not in MEL_LOGS:
        raise ValueError(f"log must be None, 'ln', 'log10' or 'db', got {log!r}")
    if log is not None and not (math.isfinite(float(amin)) and float(amin) > 0):
        raise ValueError(f"amin must be finite and > 0, got {amin}")
    if not (math.isfinite(float(ref)) and float(ref) > 0):
        raise ValueError(f"ref must be finite and > 0, got {ref}")
    if top_db is not None and (log != "db" or not float(top_db) >= 0):
        raise ValueError("top_db needs log='db' and a value >= 0")
    W = mel_filterbank(int(n_fft) // 2 + 1, f_min, float(sample_rate) / 2 if f_max is None else f_max, n_mels, sample_rate, norm, mel_scale)
    mult = {None: 0.0, "ln": 1.0, "log10": 1.0 / math.log(10.0), "db": (10.0 if power == 2 else 20.0) / math.log(10.0)}[log]
    p = _bandspec_plan(x, W, n_fft, hop_length, win_length, window, center, pad_mode, real)
    y = p.forward(x.contiguous(), power, normalized, mult, float(amin) if log is not None else 0.0)
    if log == "db":
        if float(ref) != 1.0:
            y -= mult * math.log(float(ref))
        if top_db is not None and y.numel():
            y = y.maximum(y.amax(dim=(-2, -1), keepdim=True) - float(top_db))
    return y


def mfcc(x, sample_rate, n_mfcc=40, n_fft=400, n_mels=128, f_min=0.0, f_max=None, hop_length=None, win_length=None, window=None,
         center=True, pad_mode="reflect", mel_scale="htk", mel_norm=None, amin=1e-10, ref=1.0, top_db=80.0, norm="ortho"):
    """torchaudio.transforms.MFCC: the dB mel power spectrogram (mel_spectrogram(..., power=2, log="db", amin, ref, top_db); mel_norm is
    its `norm`) followed by dct(type=2, norm=norm) along the band axis, truncated to n_mfcc coefficients -> (..., frames, n_mfcc).  A
    composition of the two calls: no kernel of its own."""
    n_mfcc = int(n_mfcc)
    if not 1 <= n_mfcc <= int(n_mels):
        raise ValueError(f"need 1 <= n_mfcc <= n_mels, got {n_mfcc}, {n_mels}")
    y = mel_spectrogram(x, sample_rate, n_fft, n_mels, f_min, f_max, hop_length, win_length, window, center, pad_mode, 2.0, False, mel_norm,
                        mel_scale, "db", amin, ref, top_db)
    return dct(y, 2, norm, -1)[..., :n_mfcc].contiguous()


class Hilbert(_Handle):
    """Batched analytic signal and envelope (include/fourier.h, fourier_hip_hilbert_*) on device memory: of rows of N reals x,
    z = ifft(fft(x) * m) with m = 1 at bin 0 and (N even) N/2, 2 between them and 0 above -- scipy.signal.hilbert(x), N complex values a
    row with Re z = x -- or the envelope |z|, N reals a row.  The envelope is abs(scipy.signal.hilbert(x)); it is NOT
    scipy.signal.envelope, which filters and returns a residual as well."""

    _prefix = "fourier_hip_hilbert_"
    _destroy = "fourier_hip_hilbert_destroy"

    def __init__(self, size, real="f32", device=-1):
        if int(size) < 1:
            raise ValueError(f"need size >= 1, got {size}")
        self._create(real, f"analytic-signal plan of size {size}", int(size), int(device))
        self._n = int(size)

    def size(self):
        return self._n

    def set_option(self, key, value):
        """"fusion": 1 = the one-launch kernel where the length has one (2^11 ... 2^15, f64 ... 2^14), 0 (default) = the composed route
        (real forward transform, expand sweep, inverse transform)."""
        self._call("set_option", key.encode(), int(value))

    def analytic_ptr(self, d_in, d_out, batch, stream=0):
        """`batch` rows of N reals at d_in -> `batch` rows of N complex values at d_out (no overlap), enqueued on `stream`."""
        self._call("analytic", d_in, d_out, int(batch), stream)

    def envelope_ptr(self, d_in, d_out, batch, stream=0):
        """`batch` rows of N reals at d_in -> `batch` rows of N reals at d_out (d_out may be d_in), enqueued on `stream`."""
        self._call("envelope", d_in, d_out, int(batch), stream)

    def _run(self, x, out, complex_out):
        import torch

        rdt, cdt = _torch_dtypes(self.real)
        _require_cuda(x, rdt)
        if x.dim() == 0 or x.shape[-1] != self._n:
            raise ValueError(f"last dimension must be {self._n}, got {tuple(x.shape)}")
        if out is None:
            out = torch.empty(x.shape, dtype=cdt if complex_out else rdt, device=x.device)
        elif complex_out or out is not x:
            _require_out(out, x.shape, cdt if complex_out else rdt, x.device)
        batch = x.numel() // self._n
        if batch:
            (self.analytic_ptr if complex_out else self.envelope_ptr)(x.data_ptr(), out.data_ptr(), batch, _stream(x))
        return out

    def analytic(self, x, out=None):
        """Contiguous (..., N) float32 / float64 CUDA tensor -> a new complex tensor of the same shape, scipy.signal.hilbert along the
        last axis, or `out` (which may not overlap `x`), on the current stream."""
        return self._run(x, out, True)

    def envelope(self, x, out=None):
        """... -> a new real tensor of the same shape, abs(scipy.signal.hilbert(x)), or `out` (which may be `x`).  Not
        scipy.signal.envelope."""
        return self._run(x, out, False)


def create_hilbert_f32(size, device=-1):
    return Hilbert(size, "f32", device)


def create_hilbert_f64(size, device=-1):
    return Hilbert(size, "f64", device)


def _hilbert(x, n, dim, out, complex_out):
    import torch

    if not (_is_torch(x) and x.is_cuda and x.dtype in (torch.float32, torch.float64)):
        raise TypeError("expected a CUDA float32 / float64 tensor")
    if x.dim() == 0:
        raise ValueError("expected at least one dimension")
    d = _normalise_dims(x.dim(), (dim,))[0]
    length = int(x.shape[d]) if n is None else int(n)
    if length < 1:
        raise ValueError(f"the transformed dimension must have length >= 1, got {length}")
    real = _precision(x.dtype)[0]
    shape = tuple(x.shape[:d]) + (length,) + tuple(x.shape[d + 1:])
    odt = _torch_dtypes(real)[1 if complex_out else 0]
    if out is not None and not (out is x and not complex_out):
        if not (_is_torch(out) and out.is_cuda and out.dtype == odt and tuple(out.shape) == shape and out.device == x.device):
            raise TypeError(f"out must be a CUDA {_names((odt,))} tensor of shape {shape} on the input's device")
    plan = _cached_plan(Hilbert, length, real, int(_device_index(x)))
    run = plan.analytic if complex_out else plan.envelope
    if d == x.dim() - 1 and length == x.shape[d] and x.is_contiguous() and (out is None or out.is_contiguous()):
        return run(x, out)
    # any other dim, layout or length: a torch copy that makes the axis last, contiguous and `length` long (zero-padded or truncated)
    src = x.movedim(d, -1)[..., :length]
    if length > src.shape[-1]:
        src = torch.nn.functional.pad(src, (0, length - src.shape[-1]))
    res = run(src.contiguous()).movedim(-1, d)
    if out is None:
        return res.contiguous()
    out.copy_(res)
    return out


def hilbert(x, N=None, dim=-1, out=None):
    """scipy.signal.hilbert(x, N, axis=dim) of a float32 / float64 CUDA tensor on the current stream: the analytic signal, complex, whose
    real part is x.  `N` zero-pads or truncates the axis first (a torch copy).  Returns a new tensor or `out`.  Only the last dimension of
    a contiguous tensor is native (one cached Hilbert handle per (N, dtype, device)); any other `dim` is moved last with a torch copy."""
    return _hilbert(x, N, dim, out, True)


def envelope(x, dim=-1, out=None):
    """abs(scipy.signal.hilbert(x, axis=dim)) of a float32 / float64 CUDA tensor on the current stream, without writing the analytic
    signal; returns a new tensor or `out`, which may be `x`.  NOT scipy.signal.envelope (which band-limits and returns a residual)."""
    return _hilbert(x, None, dim, out, False)


class CrossCorrelation(_Handle):
    """Batched pairwise cross-correlation and GCC-PHAT (include/fourier.h, fourier_hip_xcorr_*) on device memory: of rows x[b], y[b] of
    n values, zero-extended to the transform length `length` = L >= n,
        r[b, l] = sum_t conj(x[b, t]) y[b, (t + l) mod L],    out[b, j] = r[b, (lag_first + j) mod L],  j < lags,
    `lags` values a row.  L >= 2n - 1 with lag_first = -(n - 1), lags = 2n - 1 is numpy.correlate(y, x, "full") (mind the order: a peak
    at lag l > 0 means that y lags x by l samples); L == n with lag_first = 0, lags = L is the circular correlation.  Real rows
    (real_data=True, the default) give real output, complex rows complex output.  Option "weighting" = 1 is the phase transform
    (GCC-PHAT): every bin of conj(X) Y divided by |X| |Y|, exactly 0 where either is 0."""

    _prefix = "fourier_hip_xcorr_"
    _destroy = "fourier_hip_xcorr_destroy"

    def __init__(self, n, length, lag_first, lags, real="f32", real_data=True, device=-1):
        n, length, lag_first, lags = int(n), int(length), int(lag_first), int(lags)
        if not 1 <= n <= length:
            raise ValueError(f"need 1 <= n <= length, got {n}, {length}")
        if not 1 <= lags <= length:
            raise ValueError(f"need 1 <= lags <= length, got {lags}, {length}")
        if abs(lag_first) >= length:
            raise ValueError(f"need |lag_first| < length, got {lag_first}, {length}")
        self._create(real, f"cross-correlation plan of {n} values in {length}", n, length, lag_first, lags, int(bool(real_data)), int(device))
        self._n, self._l, self._first, self._lags, self.real_data = n, length, lag_first, lags, bool(real_data)

    def size(self):
        return self._n

    def length(self):
        return self._l

    def lag_first(self):
        return self._first

    def lags(self):
        return self._lags

    def set_option(self, key, value):
        """"fusion": 1 (default) = the one-launch kernel where the library has one (real rows, f64, no weighting, length 2^11 ... 2^14),
        0 = the composed route.  "weighting": 0 (default) = none, 1 = PHAT."""
        self._call("set_option", key.encode(), int(value), message=f"bad option {key}={value}")

    def correlate_ptr(self, d_x, d_y, d_out, batch, stream=0):
        """`batch` rows of n values at d_x and at d_y (which may be the same: the autocorrelation) -> `batch` rows of lags() values at
        d_out, which may overlap neither, enqueued on `stream`."""
        self._call("correlate", d_x, d_y, d_out, int(batch), stream)

    def correlate(self, x, y, out=None):
        """Contiguous (..., n) CUDA tensors of one shape, float (real_data) or complex of the handle's precision -> a new (..., lags)
        tensor of the same dtype, or `out` (which may overlap neither input), on the current stream.  `y` may be `x`."""
        import torch

        rdt, cdt = _torch_dtypes(self.real)
        dt = rdt if self.real_data else cdt
        _require_cuda(x, dt)
        _require_cuda(y, dt)
        if tuple(x.shape) != tuple(y.shape) or x.device != y.device:
            raise ValueError(f"x and y must have one shape and device, got {tuple(x.shape)} and {tuple(y.shape)}")
        if x.dim() == 0 or x.shape[-1] != self._n:
            raise ValueError(f"last dimension must be {self._n}, got {tuple(x.shape)}")
        shape = tuple(x.shape[:-1]) + (self._lags,)
        if out is None:
            out = torch.empty(shape, dtype=dt, device=x.device)
        else:
            _require_out(out, shape, dt, x.device)
        batch = x.numel() // self._n
        if batch:
            self.correlate_ptr(x.data_ptr(), y.data_ptr(), out.data_ptr(), batch, _stream(x))
        return out


def create_xcorr_f32(n, length, lag_first, lags, real_data=True, device=-1):
    return CrossCorrelation(n, length, lag_first, lags, "f32", real_data, device)


def create_xcorr_f64(n, length, lag_first, lags, real_data=True, device=-1):
    return CrossCorrelation(n, length, lag_first, lags, "f64", real_data, device)


def _xcorr_window(n, max_lag, mode):
    """(transform length, lag_first, lags) of xcorr's output"""
    if mode not in ("linear", "circular"):
        raise ValueError(f'mode must be "linear" or "circular", got {mode!r}')
    if max_lag is not None:
        max_lag = int(max_lag)
        if max_lag < 0:
            raise ValueError(f"need max_lag >= 0, got {max_lag}")
    if mode == "circular":
        if max_lag is None:
            return n, 0, n
        if 2 * max_lag + 1 > n:
            raise ValueError(f"need 2 max_lag + 1 <= n in circular mode, got {max_lag}, {n}")
        return n, -max_lag, 2 * max_lag + 1
    if max_lag is None:
        max_lag = n - 1
    if max_lag > n - 1:
        raise ValueError(f"need max_lag <= n - 1, got {max_lag}, {n}")
    length = 1
    while length < n + max_lag:  # no wrap inside the window: L - max_lag > n - 1
        length *= 2
    return length, -max_lag, 2 * max_lag + 1


def correlation_lags(n, max_lag=None, mode="linear"):
    """The lag of every output column of xcorr / gcc_phat for rows of n values: -max_lag ... max_lag, or (circular mode without max_lag)
    0 ... n - 1 in the raw order, where lag l >= n / 2 is the negative lag l - n.  A numpy int64 array."""
    import numpy as np

    _, first, lags = _xcorr_window(int(n), max_lag, mode)
    return np.arange(first, first + lags, dtype=np.int64)


def xcorr(x, y, max_lag=None, mode="linear", weighting=None, dim=-1, out=None):
    """Cross-correlation of the rows of two CUDA tensors of one shape and dtype (float32 / float64: real output; complex64 / complex128:
    complex output) along `dim`, on the current stream: out[..., j] = sum_t conj(x[t]) y[t + lag_j], lag_j = correlation_lags(n,
    max_lag, mode)[j].  mode="linear" (zero-extended, transform length next_pow2(n + max_lag), max_lag defaults to n - 1): lags
    -max_lag ... max_lag, numpy.correlate(y, x, "full") for the default.  mode="circular" (transform length n): the raw order 0 ... n - 1
    when max_lag is None, else the centred window with 2 max_lag + 1 <= n.  weighting=None, or "phat" for the phase transform.  Returns
    a new tensor or `out`.  Only the last dimension of contiguous tensors is native; any other `dim` or layout is moved last with a
    torch copy.  One cached CrossCorrelation handle per (n, window, dtype, device) and weighting."""
    import torch

    if not (_is_torch(x) and x.is_cuda and _precision(x.dtype) is not None):
        raise TypeError("expected CUDA float32 / float64 / complex64 / complex128 tensors")
    if not (_is_torch(y) and y.is_cuda and y.dtype == x.dtype and y.device == x.device):
        raise TypeError("y must be a CUDA tensor of x's dtype on x's device")
    if weighting not in (None, "phat"):
        raise ValueError(f'weighting must be None or "phat", got {weighting!r}')
    if tuple(x.shape) != tuple(y.shape):
        raise ValueError(f"x and y must have one shape, got {tuple(x.shape)} and {tuple(y.shape)}")
    if x.dim() == 0:
        raise ValueError("expected at least one dimension")
    d = _normalise_dims(x.dim(), (dim,))[0]
    n = int(x.shape[d])
    if n < 1:
        raise ValueError("the correlated dimension must have length >= 1")
    length, first, lags = _xcorr_window(n, max_lag, mode)
    real, real_data = _precision(x.dtype)
    shape = tuple(x.shape[:d]) + (lags,) + tuple(x.shape[d + 1:])
    if out is not None and not (_is_torch(out) and out.is_cuda and out.dtype == x.dtype and tuple(out.shape) == shape and out.device == x.device):
        raise TypeError(f"out must be a CUDA {_names((x.dtype,))} tensor of shape {shape} on the input's device")
    phat = weighting == "phat"
    plan = _cached_plan(_weighted_xcorr, n, length, first, lags, real, real_data, int(_device_index(x)), phat)
    if d == x.dim() - 1 and x.is_contiguous() and y.is_contiguous() and (out is None or out.is_contiguous()):
        return plan.correlate(x, y, out)
    xs = x.movedim(d, -1).contiguous()
    res = plan.correlate(xs, xs if y is x else y.movedim(d, -1).contiguous()).movedim(-1, d)
    if out is None:
        return res.contiguous()
    out.copy_(res)
    return out


def _weighted_xcorr(n, length, first, lags, real, real_data, device, phat):
    plan = CrossCorrelation(n, length, first, lags, real, real_data, device)
    plan.set_option("weighting", int(phat))
    return plan


def gcc_phat(x, y, max_lag=None, mode="linear", dim=-1, out=None):
    """xcorr(x, y, max_lag, mode, weighting="phat", dim=dim, out=out): the generalized cross-correlation with phase transform, whose
    peak is at the lag by which y trails x."""
    return xcorr(x, y, max_lag, mode, "phat", dim, out)


class Delay(_Handle):
    """Batched fractional delay and delay-and-sum (include/fourier.h, fourier_hip_delay_*) on device memory: rows of n values,
    zero-extended to the transform length `length` = L >= n, are delayed by one delay per row (in samples, any finite real, read from
    DEVICE memory), optionally weighted, and summed over groups of `channels` = C consecutive rows:
        Y[g] = sum_c w[gC + c] fft(x[gC + c], L) m(., d[gC + c]),    out[g] = ifft(Y[g])[:n],    m(k, d) = exp(-2 pi i k d / L)
    with signed bin indices k and cos(pi d) at the Nyquist bin.  A POSITIVE delay delays: out[t] = x[t - d]; to align a channel that
    arrived late by tau pass -tau.  The shift is circular over L: L >= n + ceil(max |d|) is the linear delay with zeros shifting in,
    L == n the circular shift.  Real rows (real_data=True, the default) give real output, complex rows complex output."""

    _prefix = "fourier_hip_delay_"
    _destroy = "fourier_hip_delay_destroy"

    def __init__(self, n, length, real="f32", real_data=True, channels=1, device=-1):
        n, length, channels = int(n), int(length), int(channels)
        if not 1 <= n <= length:
            raise ValueError(f"need 1 <= n <= length, got {n}, {length}")
        if channels < 1:
            raise ValueError(f"need channels >= 1, got {channels}")
        self._create(real, f"delay plan of {n} values in {length}, {channels} channels", n, length, channels, int(bool(real_data)), int(device))
        self._n, self._l, self._c, self.real_data = n, length, channels, bool(real_data)

    def size(self):
        return self._n

    def length(self):
        return self._l

    def channels(self):
        return self._c

    def set_option(self, key, value):
        """"fusion": 1 (default) = the one-launch kernel where the library has one (real rows, one channel, length 2^11 ... 2^15, f64
        ... 2^14), 0 = the composed route."""
        self._call("set_option", key.encode(), int(value), message=f"bad option {key}={value}")

    def apply_ptr(self, d_in, d_delays, d_weights, d_out, batch, stream=0):
        """`batch` rows of n values at d_in, `batch` delays at d_delays and `batch` weights at d_weights (None or 0: every weight 1), all
        of the handle's real type on the device -> batch / channels() rows of n values at d_out (d_in allowed when channels() == 1),
        enqueued on `stream`."""
        self._call("apply", d_in, d_delays, d_weights or None, d_out, int(batch), stream)

    def apply(self, x, delays, weights=None, out=None):
        """A contiguous (..., n) CUDA tensor, float (real_data) or complex of the handle's precision, whose row count is a multiple of
        channels(); `delays` and `weights` (optional) contiguous real CUDA tensors with one element per row of x -> a new tensor, or
        `out` (which may be `x` when channels() == 1): shape x.shape for one channel, else (rows / channels, n), on the current stream."""
        import torch

        rdt, cdt = _torch_dtypes(self.real)
        dt = rdt if self.real_data else cdt
        _require_cuda(x, dt)
        _require_cuda(delays, rdt)
        if weights is not None:
            _require_cuda(weights, rdt)
        if x.dim() == 0 or x.shape[-1] != self._n:
            raise ValueError(f"last dimension must be {self._n}, got {tuple(x.shape)}")
        batch = x.numel() // self._n
        if batch % self._c:
            raise ValueError(f"{batch} rows are not a multiple of {self._c} channels")
        for name, t in (("delays", delays), ("weights", weights)):
            if t is not None and (t.numel() != batch or t.device != x.device):
                raise ValueError(f"{name} must hold one element per row of x ({batch}) on its device, got {tuple(t.shape)}")
        shape = tuple(x.shape) if self._c == 1 else (batch // self._c, self._n)
        if out is None:
            out = torch.empty(shape, dtype=dt, device=x.device)
        else:
            _require_out(out, shape, dt, x.device)
            a0, b0 = x.data_ptr(), out.data_ptr()
            nin, nout = x.numel() * x.element_size(), out.numel() * out.element_size()
            if (a0 != b0 or self._c > 1) and a0 < b0 + nout and b0 < a0 + nin:
                raise ValueError("input and output overlap" + (" partially" if self._c == 1 else ""))
        if batch:
            self.apply_ptr(x.data_ptr(), delays.data_ptr(), None if weights is None else weights.data_ptr(), out.data_ptr(), batch, _stream(x))
        return out


def create_delay_f32(n, length, real_data=True, channels=1, device=-1):
    return Delay(n, length, "f32", real_data, channels, device)


def create_delay_f64(n, length, real_data=True, channels=1, device=-1):
    return Delay(n, length, "f64", real_data, channels, device)


def _delay_rows(x, lead, delays, weights, length, channels, out, out_shape):
    """fractional_delay / delay_and_sum: one value of `delays` (and `weights`) per row of x, broadcast over `lead` on the device"""
    import torch

    if not (_is_torch(x) and x.is_cuda and _precision(x.dtype) is not None):
        raise TypeError("expected a CUDA float32 / float64 / complex64 / complex128 tensor")
    real, real_data = _precision(x.dtype)
    rdt = _torch_dtypes(real)[0]
    n = int(x.shape[-1])
    if n < 1:
        raise ValueError("the delayed dimension must have length >= 1")
    length = n if length is None else int(length)
    if length < n:
        raise ValueError(f"need length >= n, got {length}, {n}")

    def per_row(v, name):
        if _is_torch(v):
            if not (v.is_cuda and v.device == x.device and v.dtype == rdt):
                raise TypeError(f"{name} must be a CUDA {_names((rdt,))} tensor on x's device, or a Python number")
        elif isinstance(v, (int, float)):
            v = torch.full((), float(v), dtype=rdt, device=x.device)  # broadcast on the device
        else:
            raise TypeError(f"{name} must be a CUDA {_names((rdt,))} tensor on x's device, or a Python number")
        try:
            return v.expand(lead).contiguous()
        except RuntimeError:
            raise ValueError(f"{name} of shape {tuple(v.shape)} do not broadcast to {tuple(lead)}") from None

    d = per_row(delays, "delays")
    w = None if weights is None else per_row(weights, "weights")
    if out is not None and not (_is_torch(out) and out.is_cuda and out.dtype == x.dtype and tuple(out.shape) == tuple(out_shape)
                                and out.device == x.device and out.is_contiguous()):
        raise TypeError(f"out must be a contiguous CUDA {_names((x.dtype,))} tensor of shape {tuple(out_shape)} on the input's device")
    plan = _cached_plan(Delay, n, length, real, real_data, channels, int(_device_index(x)))
    res = plan.apply(x.contiguous().view(-1, n), d, w, None if out is None else out.view(-1, n))
    return out if out is not None else res.view(out_shape)


def fractional_delay(x, delays, length=None, out=None):
    """The rows of a CUDA tensor `x` of shape (..., n) (float32 / float64: real output; complex64 / complex128: complex output), each
    delayed by its own number of samples, on the current stream: out[..., t] = x[..., t - d] by the band-limited (Fourier)
    interpolation of the row.  `delays`: a real CUDA tensor of x's precision broadcastable to x.shape[:-1], or a Python number (it is
    broadcast on the device; nothing is copied to the host either way).  A positive delay delays.  `length` is the transform length
    L >= n over which the shift is circular: length=None means L = n, the CIRCULAR shift (what leaves on the right comes back on the
    left); pass L >= n + ceil(max |d|) for the linear delay with zeros shifting in.  Returns a new tensor of x's shape, or `out`
    (which may be `x`).  One cached Delay handle per (n, length, dtype, device)."""
    if _is_torch(x) and x.dim() == 0:
        raise ValueError("expected at least one dimension")
    shape = tuple(x.shape) if _is_torch(x) else ()
    return _delay_rows(x, shape[:-1], delays, None, length, 1, out, shape)


def delay_and_sum(x, delays, weights=None, length=None, out=None):
    """Delay-and-sum beamforming of a CUDA tensor `x` of shape (..., C, n): out[..., t] = sum_c weights[..., c] x[..., c, t -
    delays[..., c]], shape (..., n), on the current stream.  `delays` and `weights` (None: every weight 1, a plain sum and not a
    mean): real CUDA tensors of x's precision broadcastable to x.shape[:-1], or Python numbers.  The channels are summed on their
    spectra: C forward transforms and ONE inverse a group.  A positive delay delays; to align a channel that arrived late by tau pass
    -tau.  `length` as in fractional_delay: None means L = n, the CIRCULAR shift.  Returns a new tensor or `out` (which may not
    overlap `x`).  One cached Delay handle per (n, length, C, dtype, device)."""
    if _is_torch(x) and x.dim() < 2:
        raise ValueError("expected at least two dimensions (..., C, n)")
    shape = tuple(x.shape) if _is_torch(x) else (1, 1)
    if shape[-2] < 1:
        raise ValueError("expected at least one channel")
    return _delay_rows(x, shape[:-1], delays, weights, length, shape[-2], out, shape[:-2] + shape[-1:])


class Cepstrum(_Handle):
    """Batched real cepstrum and minimum-phase reconstruction (include/fourier.h, fourier_hip_cepstrum_*) on device memory: rows of n
    reals, zero-extended to the transform length `length` = L >= n.  With X = fft(x, L) and the per-call reals log_mult != 0 and
    log_floor >= 0, g = log_mult ln(max(|X|, log_floor)) (the accurate logarithm) and
        mode 0 (Cepstrum.CEPSTRUM)       out = ifft(g)[:outputs]
        mode 1 (Cepstrum.MINIMUM_PHASE)  c = ifft(g) folded onto the quefrencies 0 ... L/2 (weights 1, 2 ... 2, 1 at even L), C = fft(.),
                                         out = Re ifft(exp(C))[:outputs]
    Mode 1 with log_mult = 1 is scipy.signal.minimum_phase(x, method="homomorphic", n_fft=L, half=False), with log_mult = 0.5 its
    half=True, up to two documented deviations: the floor is log_floor applied with max (scipy adds 1e-7 x the smallest positive |X|)
    and at even L quefrency L/2 keeps weight 1 (scipy: 0).  log_floor = 0 on a bin that is exactly 0 makes that row's output not
    finite and touches nothing else."""

    _prefix = "fourier_hip_cepstrum_"
    _destroy = "fourier_hip_cepstrum_destroy"
    CEPSTRUM, MINIMUM_PHASE = 0, 1

    def __init__(self, n, length, real="f32", outputs=None, mode=0, device=-1):
        n, length = int(n), int(length)
        outputs = n if outputs is None else int(outputs)
        if not 1 <= n <= length:
            raise ValueError(f"need 1 <= n <= length, got {n}, {length}")
        if not 1 <= outputs <= length:
            raise ValueError(f"need 1 <= outputs <= length, got {outputs}, {length}")
        if mode not in (0, 1):
            raise ValueError(f"mode is 0 (cepstrum) or 1 (minimum phase), got {mode}")
        self._create(real, f"cepstrum plan of {n} values in {length}, {outputs} outputs, mode {mode}", n, length, outputs, int(mode), int(device))
        self._n, self._l, self._m, self._mode = n, length, outputs, int(mode)

    def size(self):
        return self._n

    def length(self):
        return self._l

    def outputs(self):
        return self._m

    def mode(self):
        return self._mode

    def set_option(self, key, value):
        """"fusion": 1 (default) = the one-launch kernel where the library has one (length 2^11 ... 2^15, f64 ... 2^14; the f32
        minimum-phase row at 2^11, 2^12 and 2^14 only), 0 = the composed route."""
        self._call("set_option", key.encode(), int(value), message=f"bad option {key}={value}")

    def apply_ptr(self, d_in, d_out, batch, log_mult=1.0, log_floor=0.0, stream=0):
        """`batch` rows of n reals of the handle's type at d_in -> `batch` rows of outputs() reals at d_out (d_in allowed where
        outputs() == n), enqueued on `stream`."""
        self._call("apply", d_in, d_out, int(batch), float(log_mult), float(log_floor), stream)

    def apply(self, x, log_mult=1.0, log_floor=0.0, out=None):
        """A contiguous (..., n) CUDA float tensor of the handle's precision -> a new tensor of shape (..., outputs()), or `out` (which
        may be `x` where outputs() == n), on the current stream."""
        import torch

        rdt = _torch_dtypes(self.real)[0]
        _require_cuda(x, rdt)
        if x.dim() == 0 or x.shape[-1] != self._n:
            raise ValueError(f"last dimension must be {self._n}, got {tuple(x.shape)}")
        batch = x.numel() // self._n
        shape = tuple(x.shape[:-1]) + (self._m,)
        if out is None:
            out = torch.empty(shape, dtype=rdt, device=x.device)
        else:
            _require_out(out, shape, rdt, x.device)
            a0, b0 = x.data_ptr(), out.data_ptr()
            nin, nout = x.numel() * x.element_size(), out.numel() * out.element_size()
            if (a0 != b0 or self._m != self._n) and a0 < b0 + nout and b0 < a0 + nin:
                raise ValueError("input and output overlap")
        if batch:
            self.apply_ptr(x.data_ptr(), out.data_ptr(), batch, log_mult, log_floor, _stream(x))
        return out


def create_cepstrum_f32(n, length, outputs=None, mode=0, device=-1):
    return Cepstrum(n, length, "f32", outputs, mode, device)


def create_cepstrum_f64(n, length, outputs=None, mode=0, device=-1):
    return Cepstrum(n, length, "f64", outputs, mode, device)


def _cepstrum_rows(x, length, outputs, mode, log_mult, log_floor, out):
    if not (_is_torch(x) and x.is_cuda and _precision(x.dtype) is not None and _precision(x.dtype)[1]):
        raise TypeError("expected a CUDA float32 / float64 tensor")
    if x.dim() == 0:
        raise ValueError("expected at least one dimension")
    real = _precision(x.dtype)[0]
    n = int(x.shape[-1])
    if n < 1:
        raise ValueError("the transformed dimension must have length >= 1")
    length = n if length is None else int(length)
    if length < n:
        raise ValueError(f"need length >= n, got {length}, {n}")
    outputs = n if outputs is None else int(outputs)
    if not 1 <= outputs <= length:
        raise ValueError(f"need 1 <= outputs <= length, got {outputs}, {length}")
    shape = tuple(x.shape[:-1]) + (outputs,)
    if out is not None and not (_is_torch(out) and out.is_cuda and out.dtype == x.dtype and tuple(out.shape) == shape
                                and out.device == x.device and out.is_contiguous()):
        raise TypeError(f"out must be a contiguous CUDA {_names((x.dtype,))} tensor of shape {shape} on the input's device")
    plan = _cached_plan(Cepstrum, n, length, real, outputs, mode, int(_device_index(x)))
    return plan.apply(x.contiguous(), log_mult, log_floor, out)


def real_cepstrum(x, length=None, outputs=None, log_floor=0.0, out=None):
    """The real cepstrum irfft(log(max(|rfft(x, L)|, log_floor)))[..., :outputs] along the last axis of a CUDA float32 / float64 tensor
    `x` of shape (..., n), on the current stream.  `length` = L >= n is the transform length (None: n), `outputs` <= L the number of
    quefrencies kept (None: n).  log_floor = 0 on a bin that is exactly 0 makes that row not finite.  A non-contiguous `x` is copied.
    Returns a new tensor or `out` (which may be `x` where outputs == n).  One cached Cepstrum handle per (n, length, outputs, dtype,
    device)."""
    return _cepstrum_rows(x, length, outputs, Cepstrum.CEPSTRUM, 1.0, log_floor, out)


def minimum_phase(x, length=None, outputs=None, half=False, log_floor=0.0, out=None):
    """The minimum-phase row with the magnitude response of each row (half=True: with the square root of it) along the last axis of a
    CUDA float32 / float64 tensor `x` of shape (..., n), on the current stream: scipy.signal.minimum_phase(x, method="homomorphic",
    n_fft=length, half=half) without its truncation to (n + 1) / 2 taps -- `outputs` values are kept (None: n) -- and with the two
    documented deviations of the Cepstrum class (the floor is `log_floor` applied with max; at even length quefrency length / 2 keeps
    weight 1).  `length` >= n (None: n); choose it several times n, as scipy's default n_fft does, for an accurate result.  Returns a
    new tensor or `out` (which may be `x` where outputs == n).  One cached Cepstrum handle per (n, length, outputs, dtype, device)."""
    return _cepstrum_rows(x, length, outputs, Cepstrum.MINIMUM_PHASE, 0.5 if half else 1.0, log_floor, out)


class Nufft(_Handle):
    """Batched 1-D non-uniform FFT of types 1 and 2 (include/fourier.h, fourier_hip_nufft_*) on device memory, the points shared by
    the rows of a batch.  For n_modes = N modes k = -floor(N/2) .. ceil(N/2) - 1 and M points x_j (set_points; any finite reals, taken
    modulo 2 pi):
        to_modes  (type 1)   f[b, k] = sum_j c[b, j] exp(i isign k x_j)      (..., M) -> (..., N)
        to_points (type 2)   c[b, j] = sum_k f[b, k] exp(i isign k x_j)      (..., N) -> (..., M)
    with no scale factor; to_points with isign s is the exact adjoint of to_modes with -s.  `eps` is the requested relative accuracy:
    the kernel width is w = ceil(log10(1 / eps)) + 1, clamped to 2 .. 8 at f32 and 2 .. 16 at f64, and the relative L2 error of a call
    is about 10^(1 - w) plus the rounding of the precision.  modeord 0 stores k ascending, 1 in FFT order."""

    _prefix = "fourier_hip_nufft_"
    _destroy = "fourier_hip_nufft_destroy"

    def __init__(self, n_modes, eps=1e-6, real="f32", device=-1):
        import math

        n_modes, eps = int(n_modes), float(eps)
        if n_modes < 1:
            raise ValueError(f"need n_modes >= 1, got {n_modes}")
        if not (math.isfinite(eps) and eps > 0.0):
            raise ValueError(f"need a finite eps > 0, got {eps}")
        self._create(real, f"nufft plan of {n_modes} modes, eps {eps}", n_modes, eps, int(device))
        self._n, self.eps = n_modes, eps

    def modes(self):
        return self._n

    def points(self):
        return int(self._fn("points")(self._h))

    def set_option(self, key, value):
        """"table": 0 = the weights are evaluated in the kernels, 1 = they are read from a table written once per set_points."""
        self._call("set_option", key.encode(), int(value), message=f"bad option {key}={value}")

    def set_points_ptr(self, h_points, m, stream=0):
        """`m` float64 values at the HOST address h_points.  Waits for `stream`."""
        self._call("set_points", h_points, int(m), stream)

    def set_points(self, x):
        """A numpy array or a torch tensor (any device, any real dtype) of M points: copied to the host as float64.  Every point must be
        finite.  Replaces the points in use; waits for the current stream."""
        import numpy as np

        if _is_torch(x):
            x = x.detach().cpu().numpy()
        elif not isinstance(x, np.ndarray):
            raise TypeError("points must be a numpy array or a torch tensor")
        if x.dtype.kind not in "fiu":
            raise TypeError(f"points must be real, got {x.dtype}")
        host = np.ascontiguousarray(x, dtype=np.float64).ravel()
        if not np.isfinite(host).all():
            raise ValueError("every point must be finite")
        stream = 0
        try:
            import torch

            if torch.cuda.is_available():
                stream = torch.cuda.current_stream().cuda_stream
        except Exception:
            pass
        self.set_points_ptr(host.ctypes.data if host.size else None, host.size, stream)

    def to_modes_ptr(self, d_in, d_out, batch, isign=-1, modeord=0, stream=0):
        """`batch` rows of points() complex values at d_in -> `batch` rows of modes() complex values at d_out, enqueued on `stream`."""
        self._call("to_modes_batch", d_in, d_out, int(batch), int(isign), int(modeord), stream)

    def to_points_ptr(self, d_in, d_out, batch, isign=1, modeord=0, stream=0):
        """`batch` rows of modes() complex values at d_in -> `batch` rows of points() complex values at d_out, enqueued on `stream`."""
        self._call("to_points_batch", d_in, d_out, int(batch), int(isign), int(modeord), stream)

    def _run(self, op, x, ivals, ovals, isign, modeord, out):
        import torch

        cdt = _torch_dtypes(self.real)[1]
        _require_cuda(x, cdt)
        if x.dim() == 0 or x.shape[-1] != ivals:
            raise ValueError(f"last dimension must be {ivals}, got {tuple(x.shape)}")
        if isign not in (1, -1):
            raise ValueError(f"isign must be +1 or -1, got {isign}")
        if modeord not in (0, 1):
            raise ValueError(f"modeord must be 0 or 1, got {modeord}")
        shape = tuple(x.shape[:-1]) + (ovals,)
        batch = 1
        for s in shape[:-1]:
            batch *= int(s)
        if out is None:
            out = torch.empty(shape, dtype=cdt, device=x.device)
        else:
            _require_out(out, shape, cdt, x.device)
        if batch:
            self._call(op, x.data_ptr(), out.data_ptr(), batch, int(isign), int(modeord), _stream(x))
        return out

    def to_modes(self, c, isign=-1, modeord=0, out=None):
        """A contiguous (..., points()) complex CUDA tensor of the handle's precision -> a new (..., modes()) tensor, or `out` (which may
        not overlap `c`), on the current stream."""
        return self._run("to_modes_batch", c, self.points(), self._n, isign, modeord, out)

    def to_points(self, f, isign=1, modeord=0, out=None):
        """A contiguous (..., modes()) complex CUDA tensor of the handle's precision -> a new (..., points()) tensor, or `out` (which may
        not overlap `f`), on the current stream."""
        return self._run("to_points_batch", f, self._n, self.points(), isign, modeord, out)


def create_nufft_f32(n_modes, eps=1e-6, device=-1):
    return Nufft(n_modes, eps, "f32", device)


def create_nufft_f64(n_modes, eps=1e-6, device=-1):
    return Nufft(n_modes, eps, "f64", device)


def _nufft_plan(x, v, n_modes, eps):
    """nufft1 / nufft2: the cached handle of (n_modes, eps, precision, device) with the points `x` set"""
    if not (_is_torch(v) and v.is_cuda and _precision(v.dtype) is not None and not _precision(v.dtype)[1]):
        raise TypeError("expected a CUDA complex64 / complex128 tensor")
    if v.dim() == 0:
        raise ValueError("expected at least one dimension")
    plan = _cached_plan(Nufft, int(n_modes), float(eps), _precision(v.dtype)[0], int(_device_index(v)))
    plan.set_points(x)
    return plan


def nufft1(x, c, n_modes, eps=1e-6, isign=-1):
    """Type 1 (points to modes): f[..., k] = sum_j c[..., j] exp(i isign k x[j]), k = -floor(n_modes/2) .. ceil(n_modes/2) - 1 ascending,
    for M points `x` (numpy or torch, any device, copied to the host as float64) and a CUDA complex64 / complex128 tensor `c` of shape
    (..., M), whose leading dimensions are a batch that shares the points; on the current stream.  Returns a new (..., n_modes) tensor.
    One cached Nufft handle per (n_modes, eps, dtype, device); every call sets its points, a set-up step that waits for the stream:
    keep a Nufft of your own where the points stay."""
    plan = _nufft_plan(x, c, n_modes, eps)
    return plan.to_modes(c.contiguous(), isign)


def nufft2(x, f, eps=1e-6, isign=1):
    """Type 2 (modes to points): c[..., j] = sum_k f[..., k] exp(i isign k x[j]) for a CUDA complex64 / complex128 tensor `f` of shape
    (..., N) holding the modes k = -floor(N/2) .. ceil(N/2) - 1 ascending, and M points `x` (as for nufft1); on the current stream.
    Returns a new (..., M) tensor.  The cached handle and its set-up step are nufft1's."""
    n_modes = int(f.shape[-1]) if _is_torch(f) and f.dim() else 0
    if n_modes < 1:
        raise ValueError("the mode dimension must have length >= 1")
    plan = _nufft_plan(x, f, n_modes, eps)
    return plan.to_points(f.contiguous(), isign)


class Nufft2d(_Handle):
    """Batched 2-D non-uniform FFT of types 1 and 2 (include/fourier.h, fourier_hip_nufft2d_*) on device memory, in C order, the points
    shared by the items of a batch.  For n_modes = (N1, N2) modes k_d = -floor(N_d/2) .. ceil(N_d/2) - 1 and M points (x1_j, x2_j)
    (set_points; any finite reals, taken modulo 2 pi per coordinate; coordinate d pairs with axis d):
        to_modes  (type 1)   f[b, k1, k2] = sum_j c[b, j] exp(i isign (k1 x1_j + k2 x2_j))        (..., M) -> (..., N1, N2)
        to_points (type 2)   c[b, j] = sum_{k1,k2} f[b, k1, k2] exp(i isign (k1 x1_j + k2 x2_j))  (..., N1, N2) -> (..., M)
    with no scale factor; to_points with isign s is the exact adjoint of to_modes with -s.  `eps` is the requested relative accuracy:
    the kernel width is w = ceil(log10(1 / eps)) + 1 for both axes, clamped to 2 .. 8 at f32 and 2 .. 16 at f64, and the relative L2
    error of a call is about 2 x 10^(1 - w) plus the rounding of the precision.  modeord 0 stores both axes with k ascending, 1 both in
    FFT order."""

    _prefix = "fourier_hip_nufft2d_"
    _destroy = "fourier_hip_nufft2d_destroy"

    def __init__(self, n_modes, eps=1e-6, real="f32", device=-1):
        import math

        try:
            n1, n2 = (int(v) for v in n_modes)
        except (TypeError, ValueError):
            raise ValueError(f"need n_modes = (n1, n2), got {n_modes!r}") from None
        eps = float(eps)
        if n1 < 1 or n2 < 1:
            raise ValueError(f"need n1, n2 >= 1, got {(n1, n2)}")
        if not (math.isfinite(eps) and eps > 0.0):
            raise ValueError(f"need a finite eps > 0, got {eps}")
        self._create(real, f"nufft2d plan of {n1} x {n2} modes, eps {eps}", n1, n2, eps, int(device))
        self._n, self.eps = (n1, n2), eps

    def modes(self):
        return self._n

    def points(self):
        return int(self._fn("points")(self._h))

    def set_option(self, key, value):
        """"table": 0 = the weights are evaluated in the kernels, 1 = they are read from a table written once per set_points."""
        self._call("set_option", key.encode(), int(value), message=f"bad option {key}={value}")

    def set_points_ptr(self, h_x1, h_x2, m, stream=0):
        """`m` float64 values at each of the HOST addresses h_x1, h_x2.  Waits for `stream`."""
        self._call("set_points", h_x1, h_x2, int(m), stream)

    def set_points(self, x1, x2):
        """Two numpy arrays or torch tensors (any device, any real dtype) of M coordinates each: copied to the host as float64.  Every
        coordinate must be finite.  Replaces the points in use; waits for the current stream."""
        import numpy as np

        hosts = []
        for x in (x1, x2):
            if _is_torch(x):
                x = x.detach().cpu().numpy()
            elif not isinstance(x, np.ndarray):
                raise TypeError("points must be numpy arrays or torch tensors")
            if x.dtype.kind not in "fiu":
                raise TypeError(f"points must be real, got {x.dtype}")
            hosts.append(np.ascontiguousarray(x, dtype=np.float64).ravel())
        if hosts[0].size != hosts[1].size:
            raise ValueError(f"x1 and x2 must have the same number of points, got {hosts[0].size} and {hosts[1].size}")
        if not (np.isfinite(hosts[0]).all() and np.isfinite(hosts[1]).all()):
            raise ValueError("every point must be finite")
        stream = 0
        try:
            import torch

            if torch.cuda.is_available():
                stream = torch.cuda.current_stream().cuda_stream
        except Exception:
            pass
        m = hosts[0].size
        self.set_points_ptr(hosts[0].ctypes.data if m else None, hosts[1].ctypes.data if m else None, m, stream)

    def to_modes_ptr(self, d_in, d_out, batch, isign=-1, modeord=0, stream=0):
        """`batch` rows of points() complex values at d_in -> `batch` items of N1 x N2 complex values at d_out, enqueued on `stream`."""
        self._call("to_modes_batch", d_in, d_out, int(batch), int(isign), int(modeord), stream)

    def to_points_ptr(self, d_in, d_out, batch, isign=1, modeord=0, stream=0):
        """`batch` items of N1 x N2 complex values at d_in -> `batch` rows of points() complex values at d_out, enqueued on `stream`."""
        self._call("to_points_batch", d_in, d_out, int(batch), int(isign), int(modeord), stream)

    def _run(self, op, x, itail, otail, isign, modeord, out):
        import torch

        cdt = _torch_dtypes(self.real)[1]
        _require_cuda(x, cdt)
        if x.dim() < len(itail) or tuple(x.shape[x.dim() - len(itail):]) != itail:
            raise ValueError(f"trailing dimensions must be {itail}, got {tuple(x.shape)}")
        if isign not in (1, -1):
            raise ValueError(f"isign must be +1 or -1, got {isign}")
        if modeord not in (0, 1):
            raise ValueError(f"modeord must be 0 or 1, got {modeord}")
        lead = tuple(x.shape[:x.dim() - len(itail)])
        shape = lead + otail
        batch = 1
        for s in lead:
            batch *= int(s)
        if out is None:
            out = torch.empty(shape, dtype=cdt, device=x.device)
        else:
            _require_out(out, shape, cdt, x.device)
        if batch:
            self._call(op, x.data_ptr(), out.data_ptr(), batch, int(isign), int(modeord), _stream(x))
        return out

    def to_modes(self, c, isign=-1, modeord=0, out=None):
        """A contiguous (..., points()) complex CUDA tensor of the handle's precision -> a new (..., N1, N2) tensor, or `out` (which may
        not overlap `c`), on the current stream."""
        return self._run("to_modes_batch", c, (self.points(),), self._n, isign, modeord, out)

    def to_points(self, f, isign=1, modeord=0, out=None):
        """A contiguous (..., N1, N2) complex CUDA tensor of the handle's precision -> a new (..., points()) tensor, or `out` (which may
        not overlap `f`), on the current stream."""
        return self._run("to_points_batch", f, self._n, (self.points(),), isign, modeord, out)


def create_nufft2d_f32(n_modes, eps=1e-6, device=-1):
    return Nufft2d(n_modes, eps, "f32", device)


def create_nufft2d_f64(n_modes, eps=1e-6, device=-1):
    return Nufft2d(n_modes, eps, "f64", device)


def _nufft2d_plan(x1, x2, v, n_modes, eps):
    """nufft2d1 / nufft2d2: the cached handle of (n_modes, eps, precision, device) with the points (x1, x2) set"""
    if not (_is_torch(v) and v.is_cuda and _precision(v.dtype) is not None and not _precision(v.dtype)[1]):
        raise TypeError("expected a CUDA complex64 / complex128 tensor")
    plan = _cached_plan(Nufft2d, (int(n_modes[0]), int(n_modes[1])), float(eps), _precision(v.dtype)[0], int(_device_index(v)))
    plan.set_points(x1, x2)
    return plan


def nufft2d1(x1, x2, c, n_modes, eps=1e-6, isign=-1):
    """2-D type 1 (points to modes): f[..., k1, k2] = sum_j c[..., j] exp(i isign (k1 x1[j] + k2 x2[j])), k_d = -floor(N_d/2) ..
    ceil(N_d/2) - 1 ascending, n_modes = (N1, N2), for M points (x1, x2) (numpy or torch, any device, copied to the host as float64)
    and a CUDA complex64 / complex128 tensor `c` of shape (..., M), whose leading dimensions are a batch that shares the points; on the
    current stream.  Returns a new (..., N1, N2) tensor.  One cached Nufft2d handle per (n_modes, eps, dtype, device); every call sets
    its points, a set-up step that waits for the stream: keep a Nufft2d of your own where the points stay."""
    if not (_is_torch(c) and c.dim() >= 1):
        raise TypeError("expected a CUDA complex64 / complex128 tensor of at least one dimension")
    plan = _nufft2d_plan(x1, x2, c, n_modes, eps)
    return plan.to_modes(c.contiguous(), isign)


def nufft2d2(x1, x2, f, eps=1e-6, isign=1):
    """2-D type 2 (modes to points): c[..., j] = sum_{k1,k2} f[..., k1, k2] exp(i isign (k1 x1[j] + k2 x2[j])) for a CUDA complex64 /
    complex128 tensor `f` of shape (..., N1, N2) holding the modes ascending on both axes, and M points (x1, x2) (as for nufft2d1); on
    the current stream.  Returns a new (..., M) tensor.  The cached handle and its set-up step are nufft2d1's."""
    if not (_is_torch(f) and f.dim() >= 2 and f.shape[-1] >= 1 and f.shape[-2] >= 1):
        raise ValueError("expected a tensor whose two mode dimensions have length >= 1")
    plan = _nufft2d_plan(x1, x2, f, (int(f.shape[-2]), int(f.shape[-1])), eps)
    return plan.to_points(f.contiguous(), isign)


class Nufft3d(Nufft2d):
    """Batched 3-D non-uniform FFT of types 1 and 2 (include/fourier.h, fourier_hip_nufft3d_*) on device memory, in C order, the points
    shared by the items of a batch.  For n_modes = (N1, N2, N3) modes k_d = -floor(N_d/2) .. ceil(N_d/2) - 1 and M points
    (x1_j, x2_j, x3_j) (set_points; any finite reals, taken modulo 2 pi per coordinate; coordinate d pairs with axis d):
        to_modes  (type 1)   f[b, k1, k2, k3] = sum_j c[b, j] exp(i isign (k1 x1_j + k2 x2_j + k3 x3_j))           (..., M) -> (..., N1, N2, N3)
        to_points (type 2)   c[b, j] = sum_{k1,k2,k3} f[b, k1, k2, k3] exp(i isign (k1 x1_j + k2 x2_j + k3 x3_j))  (..., N1, N2, N3) -> (..., M)
    with no scale factor; to_points with isign s is the exact adjoint of to_modes with -s.  `eps` is the requested relative accuracy:
    the kernel width is w = ceil(log10(1 / eps)) + 1 for all three axes, clamped to 2 .. 8 at f32 and 2 .. 16 at f64, and the relative
    L2 error of a call is about 3 x 10^(1 - w) plus the rounding of the precision.  modeord 0 stores all three axes with k ascending,
    1 all three in FFT order.  The methods are Nufft2d's with a third coordinate."""

    _prefix = "fourier_hip_nufft3d_"
    _destroy = "fourier_hip_nufft3d_destroy"

    def __init__(self, n_modes, eps=1e-6, real="f32", device=-1):
        import math

        try:
            n1, n2, n3 = (int(v) for v in n_modes)
        except (TypeError, ValueError):
            raise ValueError(f"need n_modes = (n1, n2, n3), got {n_modes!r}") from None
        eps = float(eps)
        if n1 < 1 or n2 < 1 or n3 < 1:
            raise ValueError(f"need n1, n2, n3 >= 1, got {(n1, n2, n3)}")
        if not (math.isfinite(eps) and eps > 0.0):
            raise ValueError(f"need a finite eps > 0, got {eps}")
        self._create(real, f"nufft3d plan of {n1} x {n2} x {n3} modes, eps {eps}", n1, n2, n3, eps, int(device))
        self._n, self.eps = (n1, n2, n3), eps

    def set_points_ptr(self, h_x1, h_x2, h_x3, m, stream=0):
        """`m` float64 values at each of the HOST addresses h_x1, h_x2, h_x3.  Waits for `stream`."""
        self._call("set_points", h_x1, h_x2, h_x3, int(m), stream)

    def set_points(self, x1, x2, x3):
        """Three numpy arrays or torch tensors (any device, any real dtype) of M coordinates each: copied to the host as float64.  Every
        coordinate must be finite.  Replaces the points in use; waits for the current stream."""
        import numpy as np

        hosts = []
        for x in (x1, x2, x3):
            if _is_torch(x):
                x = x.detach().cpu().numpy()
            elif not isinstance(x, np.ndarray):
                raise TypeError("points must be numpy arrays or torch tensors")
            if x.dtype.kind not in "fiu":
                raise TypeError(f"points must be real, got {x.dtype}")
            hosts.append(np.ascontiguousarray(x, dtype=np.float64).ravel())
        m = hosts[0].size
        if hosts[1].size != m or hosts[2].size != m:
            raise ValueError(f"x1, x2 and x3 must have the same number of points, got {[h.size for h in hosts]}")
        if not all(np.isfinite(h).all() for h in hosts):
            raise ValueError("every point must be finite")
        stream = 0
        try:
            import torch

            if torch.cuda.is_available():
                stream = torch.cuda.current_stream().cuda_stream
        except Exception:
            pass
        self.set_points_ptr(*(h.ctypes.data if m else None for h in hosts), m, stream)


def create_nufft3d_f32(n_modes, eps=1e-6, device=-1):
    return Nufft3d(n_modes, eps, "f32", device)


def create_nufft3d_f64(n_modes, eps=1e-6, device=-1):
    return Nufft3d(n_modes, eps, "f64", device)


def _nufft3d_plan(x1, x2, x3, v, n_modes, eps):
    """nufft3d1 / nufft3d2: the cached handle of (n_modes, eps, precision, device) with the points (x1, x2, x3) set"""
    if not (_is_torch(v) and v.is_cuda and _precision(v.dtype) is not None and not _precision(v.dtype)[1]):
        raise TypeError("expected a CUDA complex64 / complex128 tensor")
    plan = _cached_plan(Nufft3d, tuple(int(n) for n in n_modes), float(eps), _precision(v.dtype)[0], int(_device_index(v)))
    plan.set_points(x1, x2, x3)
    return plan


def nufft3d1(x1, x2, x3, c, n_modes, eps=1e-6, isign=-1):
    """3-D type 1 (points to modes): f[..., k1, k2, k3] = sum_j c[..., j] exp(i isign (k1 x1[j] + k2 x2[j] + k3 x3[j])),
    k_d = -floor(N_d/2) .. ceil(N_d/2) - 1 ascending, n_modes = (N1, N2, N3), for M points (x1, x2, x3) (numpy or torch, any device,
    copied to the host as float64) and a CUDA complex64 / complex128 tensor `c` of shape (..., M), whose leading dimensions are a
    batch that shares the points; on the current stream.  Returns a new (..., N1, N2, N3) tensor.  One cached Nufft3d handle per
    (n_modes, eps, dtype, device); every call sets its points, a set-up step that waits for the stream: keep a Nufft3d of your own
    where the points stay."""
    if not (_is_torch(c) and c.dim() >= 1):
        raise TypeError("expected a CUDA complex64 / complex128 tensor of at least one dimension")
    plan = _nufft3d_plan(x1, x2, x3, c, n_modes, eps)
    return plan.to_modes(c.contiguous(), isign)


def nufft3d2(x1, x2, x3, f, eps=1e-6, isign=1):
    """3-D type 2 (modes to points): c[..., j] = sum_{k1,k2,k3} f[..., k1, k2, k3] exp(i isign (k1 x1[j] + k2 x2[j] + k3 x3[j])) for a
    CUDA complex64 / complex128 tensor `f` of shape (..., N1, N2, N3) holding the modes ascending on all three axes, and M points
    (x1, x2, x3) (as for nufft3d1); on the current stream.  Returns a new (..., M) tensor.  The cached handle and its set-up step are
    nufft3d1's."""
    if not (_is_torch(f) and f.dim() >= 3 and min(f.shape[-3:]) >= 1):
        raise ValueError("expected a tensor whose three mode dimensions have length >= 1")
    plan = _nufft3d_plan(x1, x2, x3, f, tuple(int(s) for s in f.shape[-3:]), eps)
    return plan.to_points(f.contiguous(), isign)


class Resample(_Handle):
    """Batched Fourier-domain resampling (include/fourier.h, fourier_hip_resample_*) on device memory: rows of n_in values -> rows of
    n_out values, the spectrum cut or zero-padded and transformed back -- scipy.signal.resample(x, n_out, axis=-1, window=W) with W an
    array of n_in reals in FFT order, or no window.  Real rows (real_input=True, the default) or complex rows of the handle's precision.
    ONE exception to scipy 1.15: complex rows with n_out == 2 < n_in add X[n_in - 1] into bin 1 as every other even length does (scipy's
    slice is empty there), so that complex rows with zero imaginary part agree with real rows.  scipy's `t`, domain="freq" and window
    names or callables are not offered."""

    _prefix = "fourier_hip_resample_"
    _destroy = "fourier_hip_resample_destroy"

    def __init__(self, n_in, n_out, real="f32", device=-1, real_input=True):
        n_in, n_out = int(n_in), int(n_out)
        if n_in < 1 or n_out < 1:
            raise ValueError(f"need n_in >= 1 and n_out >= 1, got {n_in}, {n_out}")
        self._create(real, f"resampling plan of {n_in} -> {n_out} values", n_in, n_out, int(bool(real_input)), int(device))
        self._n, self._m, self.real_input = n_in, n_out, bool(real_input)

    def size_in(self):
        return self._n

    def size_out(self):
        return self._m

    def set_option(self, key, value):
        """"fusion": 1 (default) = the fused untangle route (real rows, n_in and n_out both even: one sweep between the two inner
        transforms), 0 = the composed route.  Accepted without effect where there is no fused route."""
        self._call("set_option", key.encode(), int(value), message=f"bad option {key}={value}")

    def set_window_ptr(self, d_window, stream=0):
        """size_in() reals of the handle's precision at d_window, FFT order (0 / None: no window).  Waits for `stream`."""
        self._call("set_window", d_window or None, stream)

    def forward_ptr(self, d_in, d_out, batch, stream=0):
        """`batch` rows of size_in() values at d_in -> `batch` rows of size_out() values at d_out (no overlap), enqueued on `stream`."""
        self._call("forward", d_in, d_out, int(batch), stream)

    def set_window(self, window):
        """A contiguous CUDA tensor of size_in() reals of the handle's precision in FFT order (DC first), or None for no window; on the
        current stream.  The handle keeps a copy."""
        if window is None:
            return self.set_window_ptr(None)
        _require_cuda(window, _torch_dtypes(self.real)[0])
        if tuple(window.shape) != (self._n,):
            raise ValueError(f"window must have shape ({self._n},), got {tuple(window.shape)}")
        self.set_window_ptr(window.data_ptr(), _stream(window))

    def forward(self, x, out=None):
        """Contiguous (..., n_in) CUDA tensor, float (real_input) or complex of the handle's precision -> a new (..., n_out) tensor of
        the same dtype, or `out` (which may not overlap `x`), on the current stream."""
        import torch

        rdt, cdt = _torch_dtypes(self.real)
        dt = rdt if self.real_input else cdt
        _require_cuda(x, dt)
        if x.dim() == 0 or x.shape[-1] != self._n:
            raise ValueError(f"last dimension must be {self._n}, got {tuple(x.shape)}")
        shape = tuple(x.shape[:-1]) + (self._m,)
        if out is None:
            out = torch.empty(shape, dtype=dt, device=x.device)
        else:
            _require_out(out, shape, dt, x.device)
        batch = x.numel() // self._n
        if batch:
            self.forward_ptr(x.data_ptr(), out.data_ptr(), batch, _stream(x))
        return out


def create_resample_f32(n_in, n_out, real_input=True, device=-1):
    return Resample(n_in, n_out, "f32", device, real_input)


def create_resample_f64(n_in, n_out, real_input=True, device=-1):
    return Resample(n_in, n_out, "f64", device, real_input)


def resample(x, num, window=None, dim=-1, out=None):
    """scipy.signal.resample(x, num, axis=dim, window=window) of a CUDA tensor on the current stream: float32 / float64 (real rows) or
    complex64 / complex128 (complex rows); `window` is None or a CUDA tensor of x.shape[dim] reals of the same precision in FFT order.
    Returns a new tensor of the input's dtype with `num` values along `dim`, or `out`.  Only the last dimension of a contiguous tensor
    is native; any other `dim` or layout is moved last with a torch copy.  One cached Resample handle per (n_in, num, dtype, device);
    a call with a window uses a handle of its own that is not cached.  One exception to scipy 1.15: complex rows with num == 2 <
    x.shape[dim] add the bin N - 1 into bin 1, as real rows do (include/fourier.h)."""
    import torch

    if not (_is_torch(x) and x.is_cuda and _precision(x.dtype) is not None):
        raise TypeError("expected a CUDA float32 / float64 / complex64 / complex128 tensor")
    if x.dim() == 0:
        raise ValueError("expected at least one dimension")
    d = _normalise_dims(x.dim(), (dim,))[0]
    n, num = int(x.shape[d]), int(num)
    if n < 1 or num < 1:
        raise ValueError(f"the resampled dimension must have length >= 1 and num >= 1, got {n}, {num}")
    real, real_input = _precision(x.dtype)
    shape = tuple(x.shape[:d]) + (num,) + tuple(x.shape[d + 1:])
    if out is not None and not (_is_torch(out) and out.is_cuda and out.dtype == x.dtype and tuple(out.shape) == shape and out.device == x.device):
        raise TypeError(f"out must be a CUDA {_names((x.dtype,))} tensor of shape {shape} on the input's device")
    if window is None:
        plan = _cached_plan(Resample, n, num, real, int(_device_index(x)), real_input)
    else:
        if not (_is_torch(window) and window.is_cuda and window.dtype == _torch_dtypes(real)[0] and window.device == x.device):
            raise TypeError(f"window must be a CUDA {_names((_torch_dtypes(real)[0],))} tensor on the input's device")
        plan = Resample(n, num, real, int(_device_index(x)), real_input)
        plan.set_window(window.contiguous())
    if d == x.dim() - 1 and x.is_contiguous() and (out is None or out.is_contiguous()):
        return plan.forward(x, out)
    res = plan.forward(x.movedim(d, -1).contiguous()).movedim(-1, d)
    if out is None:
        return res.contiguous()
    out.copy_(res)
    return out


class Czt(_Handle):
    """Batched chirp-z transform (include/fourier.h, fourier_hip_czt_*) on device memory: of rows of n values x (complex, or reals with
    real_input=True) the m values X[k] = sum_j x[j] a**-j w**(j k), with w = w_abs exp(2 pi i w_turns) and a = a_abs exp(2 pi i a_turns)
    -- scipy.signal.czt(x, m, w, a) along the last axis.  The angles are in TURNS; w_turns=None means -1/m (with n == m, a = 1: the DFT)."""

    _prefix = "fourier_hip_czt_"
    _destroy = "fourier_hip_czt_destroy"

    def __init__(self, n, m, w_abs=1.0, w_turns=None, a_abs=1.0, a_turns=0.0, real="f32", real_input=False, device=-1):
        if int(n) < 1 or int(m) < 1:
            raise ValueError(f"need n >= 1 and m >= 1, got {n}, {m}")
        if w_turns is None:
            w_turns = -1.0 / int(m)
        pars = tuple(float(v) for v in (w_abs, w_turns, a_abs, a_turns))
        if not all(np.isfinite(pars)) or pars[0] <= 0 or pars[2] <= 0:
            raise ValueError(f"need finite parameters and positive magnitudes, got w_abs, w_turns, a_abs, a_turns = {pars}")
        self._create(real, f"chirp-z plan of {n} samples and {m} points", int(n), int(m), *pars, int(bool(real_input)), int(device))
        self._n, self._m, self.real_input = int(n), int(m), bool(real_input)

    def size(self):
        return self._n

    def points(self):
        return self._m

    def set_option(self, key, value):
        """"fusion": 1 = the one-launch kernel where max(2048, next_pow2(n + m - 1)) is at most 2^15 (f64: 2^14), 0 = the composed route
        (chirp sweep, convolution of next_pow2(n + m - 1) points, chirp sweep).  Default: 1 where next_pow2(n + m - 1) >= 2048 and the
        kernel exists, else 0."""
        self._call("set_option", key.encode(), int(value))

    def transform_ptr(self, d_in, d_out, batch, stream=0):
        """`batch` rows of n values at d_in -> `batch` rows of m complex values at d_out (no overlap), enqueued on `stream`."""
        self._call("transform", d_in, d_out, int(batch), stream)

    def transform(self, x, out=None):
        """Contiguous (..., n) CUDA tensor, complex (real_input: float) of the handle's precision -> a new complex (..., m) tensor, or
        `out` (which may not overlap `x`), on the current stream."""
        import torch

        rdt, cdt = _torch_dtypes(self.real)
        _require_cuda(x, rdt if self.real_input else cdt)
        if x.dim() == 0 or x.shape[-1] != self._n:
            raise ValueError(f"last dimension must be {self._n}, got {tuple(x.shape)}")
        shape = tuple(x.shape[:-1]) + (self._m,)
        if out is None:
            out = torch.empty(shape, dtype=cdt, device=x.device)
        else:
            _require_out(out, shape, cdt, x.device)
        batch = x.numel() // self._n
        if batch:
            self.transform_ptr(x.data_ptr(), out.data_ptr(), batch, _stream(x))
        return out


def create_czt_f32(n, m, w_abs=1.0, w_turns=None, a_abs=1.0, a_turns=0.0, real_input=False, device=-1):
    return Czt(n, m, w_abs, w_turns, a_abs, a_turns, "f32", real_input, device)


def create_czt_f64(n, m, w_abs=1.0, w_turns=None, a_abs=1.0, a_turns=0.0, real_input=False, device=-1):
    return Czt(n, m, w_abs, w_turns, a_abs, a_turns, "f64", real_input, device)


def _czt(x, m, w_abs, w_turns, a_abs, a_turns, dim, out):
    import torch

    if not (_is_torch(x) and x.is_cuda and _precision(x.dtype) is not None):
        raise TypeError("expected a CUDA float32 / float64 / complex64 / complex128 tensor")
    if x.dim() == 0:
        raise ValueError("expected at least one dimension")
    d = _normalise_dims(x.dim(), (dim,))[0]
    n = int(x.shape[d])
    m = n if m is None else int(m)
    if n < 1 or m < 1:
        raise ValueError(f"need n >= 1 and m >= 1, got {n}, {m}")
    real, real_input = _precision(x.dtype)
    shape = tuple(x.shape[:d]) + (m,) + tuple(x.shape[d + 1:])
    cdt = _torch_dtypes(real)[1]
    if out is not None and not (_is_torch(out) and out.is_cuda and out.dtype == cdt and tuple(out.shape) == shape and out.device == x.device):
        raise TypeError(f"out must be a CUDA {_names((cdt,))} tensor of shape {shape} on the input's device")
    if w_turns is None:
        w_turns = -1.0 / m
    plan = _cached_plan(Czt, n, m, float(w_abs), float(w_turns), float(a_abs), float(a_turns), real, real_input, int(_device_index(x)))
    if d == x.dim() - 1 and x.is_contiguous() and (out is None or out.is_contiguous()):
        return plan.transform(x, out)
    # any other dim or layout: a torch copy that makes the axis last and contiguous
    res = plan.transform(x.movedim(d, -1).contiguous()).movedim(-1, d)
    if out is None:
        return res.contiguous()
    out.copy_(res)
    return out


def _polar_turns(z):
    """a complex (or real) number as (magnitude, angle in turns)"""
    z = complex(z)
    return abs(z), np.angle(z) / (2.0 * np.pi)


def czt(x, m=None, w=None, a=1 + 0j, dim=-1, out=None):
    """scipy.signal.czt(x, m, w, a, axis=dim) of a float or complex CUDA tensor on the current stream: m points (default: the axis'
    length) of the z-transform at z = a w**-k; w=None means exp(-2 pi i / m), with a = 1 the DFT.  Complex `w` and `a` are converted with
    abs and angle / (2 pi); a caller who has the angles in turns keeps their precision with the Czt handle or zoom_fft.  Returns a new
    complex tensor or `out`.  Only the last dimension of a contiguous tensor is native (one cached Czt handle per parameter tuple); any
    other `dim` is moved last with a torch copy."""
    w_abs, w_turns = (1.0, None) if w is None else _polar_turns(w)
    a_abs, a_turns = _polar_turns(a)
    return _czt(x, m, w_abs, w_turns, a_abs, a_turns, dim, out)


def zoom_fft(x, fn, m=None, fs=2, endpoint=False, dim=-1, out=None):
    """scipy.signal.zoom_fft(x, fn, m, fs=fs, endpoint=endpoint, axis=dim): m points (default: the axis' length) of the DFT between the
    frequencies f1 and f2 at sample rate fs -- fn = f2 (f1 = 0) or the pair (f1, f2); endpoint=True includes f2.  The angles go to the
    handle in turns, -(f2 - f1) / (fs m) and f1 / fs, without passing through exp and atan2."""
    f1, f2 = (0.0, float(fn)) if np.ndim(fn) == 0 else (float(fn[0]), float(fn[1]))
    if np.ndim(fn) != 0 and len(fn) != 2:
        raise ValueError("fn must be a scalar or a pair (f1, f2)")
    if not _is_torch(x):
        raise TypeError("expected a CUDA float32 / float64 / complex64 / complex128 tensor")
    if x.dim() == 0:
        raise ValueError("expected at least one dimension")
    points = int(x.shape[_normalise_dims(x.dim(), (dim,))[0]]) if m is None else int(m)
    if points < 1 or (endpoint and points < 2):
        raise ValueError(f"need m >= 1 (with endpoint: m >= 2), got {points}")
    fs = float(fs)
    w_turns = -(f2 - f1) / (fs * ((points - 1) if endpoint else points))
    return _czt(x, points, 1.0, w_turns, 1.0, f1 / fs, dim, out)


class Pfb(_Handle):
    """Batched polyphase filter bank channelizer (include/fourier.h, fourier_hip_pfb_*) on device memory: of rows of `length` values
    (complex, or reals with real_input=True), frames of channels * taps values every `hop` values are folded under a prototype filter onto
    `channels` points and transformed: X[f, k] = sum_n (sum_t h[t P + n] x[f D + t P + n]) exp(-2 pi i k n / P).  Output frames x bins
    complex per row, FRAME-MAJOR; bins = channels (complex rows) or channels // 2 + 1 (real rows).  No padding, no per-frame phase
    rotation, no scale.  hop=None means channels (critically sampled).  The filter is set afterwards (set_filter; default all ones)."""

    _prefix = "fourier_hip_pfb_"
    _destroy = "fourier_hip_pfb_destroy"

    def __init__(self, channels, taps, real="f32", hop=None, real_input=False, device=-1):
        channels, taps = int(channels), int(taps)
        hop = channels if hop is None else int(hop)
        if channels < 1 or taps < 1 or hop < 1:
            raise ValueError(f"need channels >= 1, taps >= 1 and hop >= 1, got {channels}, {taps}, {hop}")
        self._create(real, f"filter bank plan of {channels} channels, {taps} taps, hop {hop}", channels, taps, hop, int(bool(real_input)),
                     int(device))
        self._p, self._t, self._hop, self.real_input = channels, taps, hop, bool(real_input)

    def channels(self):
        return self._p

    def taps(self):
        return self._t

    def hop(self):
        return self._hop

    def bins(self):
        return self._p // 2 + 1 if self.real_input else self._p

    def frames(self, length):
        """Frames of a row of `length` values; 0 where the length is invalid."""
        return int(self._fn("frames")(self._h, int(length)))

    def set_option(self, key, value):
        """"fusion": 0 = the composed route, 1 = the fused one-launch route wherever it exists (the default)."""
        self._call("set_option", key.encode(), int(value), message=f"bad option {key}={value}")

    def reserve(self, length, batch):
        """Later forward calls of at most `batch` rows of `length` values never allocate."""
        self._call("reserve", int(length), int(batch))

    def set_filter_ptr(self, d_filter, stream=0):
        """channels() * taps() reals of the handle's precision at d_filter (0 / None: all ones).  Waits for `stream`."""
        self._call("set_filter", d_filter or None, stream)

    def forward_ptr(self, d_in, d_out, length, batch, stream=0):
        """`batch` rows of `length` values at d_in -> batch x frames(length) x bins() complex at d_out, enqueued on `stream`."""
        self._call("forward", d_in, d_out, int(length), int(batch), stream)

    def set_filter(self, filter):
        """A contiguous CUDA tensor of channels() * taps() reals of the handle's precision, shape (channels * taps,) or (taps, channels),
        or None for all ones; on the current stream."""
        if filter is None:
            return self.set_filter_ptr(None)
        _require_cuda(filter, _torch_dtypes(self.real)[0])
        if tuple(filter.shape) not in ((self._p * self._t,), (self._t, self._p)):
            raise ValueError(f"filter must have shape ({self._p * self._t},) or ({self._t}, {self._p}), got {tuple(filter.shape)}")
        self.set_filter_ptr(filter.data_ptr(), _stream(filter))

    def forward(self, x, out=None):
        """Contiguous (..., length) CUDA tensor, complex (real_input: float) of the handle's precision -> a new (..., frames, bins)
        complex tensor (frame-major), or `out` (which may not overlap `x`), on the current stream."""
        import torch

        rdt, cdt = _torch_dtypes(self.real)
        _require_cuda(x, rdt if self.real_input else cdt)
        if x.dim() == 0:
            raise ValueError("expected at least one dimension")
        length = int(x.shape[-1])
        fr = self.frames(length)
        if fr == 0:
            raise ValueError(f"a row of {length} values is too short for {self._p} channels x {self._t} taps")
        shape = tuple(x.shape[:-1]) + (fr, self.bins())
        if out is None:
            out = torch.empty(shape, dtype=cdt, device=x.device)
        else:
            _require_out(out, shape, cdt, x.device)
        batch = x.numel() // length
        if batch:
            self.forward_ptr(x.data_ptr(), out.data_ptr(), length, batch, _stream(x))
        return out


def create_pfb_f32(channels, taps, hop=None, real_input=False, device=-1):
    return Pfb(channels, taps, "f32", hop, real_input, device)


def create_pfb_f64(channels, taps, hop=None, real_input=False, device=-1):
    return Pfb(channels, taps, "f64", hop, real_input, device)


def pfb_channelize(x, filter, channels, hop=None, out=None):
    """The polyphase filter bank of a CUDA tensor of shape (..., length) on the current stream: float32 / float64 rows (real input,
    channels // 2 + 1 bins) or complex64 / complex128 rows (`channels` bins); `filter` holds channels * taps reals of the same
    precision on the same device, shape (channels * taps,) or (taps, channels), or is None for all ones of one tap.  Returns
    (..., frames, bins) complex, or `out`.  Leading dimensions fold into the batch.  Handles are cached per (channels, taps, hop, dtype,
    device) and the filter is set on EVERY call; keep a Pfb to reuse one."""
    if not (_is_torch(x) and x.is_cuda and _precision(x.dtype) is not None):
        raise TypeError("expected a CUDA float32 / float64 / complex64 / complex128 tensor")
    if x.dim() == 0:
        raise ValueError("expected at least one dimension")
    real, real_input = _precision(x.dtype)
    channels = int(channels)
    if channels < 1:
        raise ValueError(f"need channels >= 1, got {channels}")
    taps = 1
    if filter is not None:
        if not (_is_torch(filter) and filter.is_cuda and filter.dtype == _torch_dtypes(real)[0] and filter.device == x.device):
            raise TypeError(f"filter must be a CUDA {_names((_torch_dtypes(real)[0],))} tensor on the input's device")
        if filter.numel() == 0 or filter.numel() % channels or (filter.dim() == 2 and filter.shape[1] != channels) or filter.dim() not in (1, 2):
            raise ValueError(f"filter must hold channels * taps values as (channels * taps,) or (taps, {channels}), got {tuple(filter.shape)}")
        taps = filter.numel() // channels
        filter = filter.contiguous()
    p = _cached_plan(Pfb, channels, taps, real, channels if hop is None else int(hop), real_input, int(_device_index(x)))
    p.set_filter(filter)
    return p.forward(x.contiguous(), out)


class Ipfb(_Handle):
    """Batched polyphase synthesis filter bank (include/fourier.h, fourier_hip_ipfb_*) on device memory, the mirror of Pfb: frames x
    bins complex values per row, FRAME-MAJOR (what Pfb.forward writes), are inverse-transformed to `channels` values each and
    overlap-added under a synthesis filter g: y[t] = sum_f g[t - f D] v[f, (t - f D) mod P] over the frames that cover t, in ascending f.
    Rows of 1 <= length <= length(frames) values out, complex, or reals with real_output=True (bins = channels // 2 + 1).  No envelope
    division, no phase rotation: reconstruction is a property of the filter pair (pfb_reconstruction_terms).  hop=None means channels.
    The filter is set afterwards (set_filter; default all ones)."""

    _prefix = "fourier_hip_ipfb_"
    _destroy = "fourier_hip_ipfb_destroy"

    def __init__(self, channels, taps, real="f32", hop=None, real_output=False, device=-1):
        channels, taps = int(channels), int(taps)
        hop = channels if hop is None else int(hop)
        if channels < 1 or taps < 1 or hop < 1:
            raise ValueError(f"need channels >= 1, taps >= 1 and hop >= 1, got {channels}, {taps}, {hop}")
        self._create(real, f"synthesis filter bank plan of {channels} channels, {taps} taps, hop {hop}", channels, taps, hop,
                     int(bool(real_output)), int(device))
        self._p, self._t, self._hop, self.real_output = channels, taps, hop, bool(real_output)

    def channels(self):
        return self._p

    def taps(self):
        return self._t

    def hop(self):
        return self._hop

    def bins(self):
        return self._p // 2 + 1 if self.real_output else self._p

    def length(self, frames):
        """(frames - 1) * hop + channels * taps, the longest row `frames` frames give; 0 where the frame count is invalid."""
        return int(self._fn("length")(self._h, int(frames)))

    def reserve(self, frames, batch):
        """Later inverse calls from at most `frames` frames and `batch` rows never allocate."""
        self._call("reserve", int(frames), int(batch))

    def set_filter_ptr(self, d_filter, stream=0):
        """channels() * taps() reals of the handle's precision at d_filter (0 / None: all ones).  Waits for `stream`."""
        self._call("set_filter", d_filter or None, stream)

    def inverse_ptr(self, d_in, d_out, frames, length, batch, stream=0):
        """batch x frames x bins() complex at d_in -> `batch` rows of `length` values at d_out, enqueued on `stream`."""
        self._call("inverse", d_in, d_out, int(frames), int(length), int(batch), stream)

    def set_filter(self, filter):
        """A contiguous CUDA tensor of channels() * taps() reals of the handle's precision, shape (channels * taps,) or (taps, channels),
        or None for all ones; on the current stream."""
        if filter is None:
            return self.set_filter_ptr(None)
        _require_cuda(filter, _torch_dtypes(self.real)[0])
        if tuple(filter.shape) not in ((self._p * self._t,), (self._t, self._p)):
            raise ValueError(f"filter must have shape ({self._p * self._t},) or ({self._t}, {self._p}), got {tuple(filter.shape)}")
        self.set_filter_ptr(filter.data_ptr(), _stream(filter))

    def inverse(self, Y, length=None, out=None):
        """Contiguous (..., frames, bins) complex CUDA tensor of the handle's precision -> a new (..., length) tensor, float where
        real_output, else complex, or `out` (which may not overlap `Y`), on the current stream.  length=None: length(frames)."""
        import torch

        rdt, cdt = _torch_dtypes(self.real)
        _require_cuda(Y, cdt)
        if Y.dim() < 2 or int(Y.shape[-1]) != self.bins():
            raise ValueError(f"expected (..., frames, {self.bins()}), got {tuple(Y.shape)}")
        frames = int(Y.shape[-2])
        full = self.length(frames)
        if full == 0:
            raise ValueError(f"{frames} frames are not a valid frame count")
        length = full if length is None else int(length)
        if not 1 <= length <= full:
            raise ValueError(f"length must be 1 ... {full} for {frames} frames, got {length}")
        shape = tuple(Y.shape[:-2]) + (length,)
        odt = rdt if self.real_output else cdt
        if out is None:
            out = torch.empty(shape, dtype=odt, device=Y.device)
        else:
            _require_out(out, shape, odt, Y.device)
        batch = Y.numel() // (frames * self.bins())
        if batch:
            self.inverse_ptr(Y.data_ptr(), out.data_ptr(), frames, length, batch, _stream(Y))
        return out


def create_ipfb_f32(channels, taps, hop=None, real_output=False, device=-1):
    return Ipfb(channels, taps, "f32", hop, real_output, device)


def create_ipfb_f64(channels, taps, hop=None, real_output=False, device=-1):
    return Ipfb(channels, taps, "f64", hop, real_output, device)


def pfb_synthesize(Y, filter, channels, hop=None, length=None, real_output=False, out=None):
    """The polyphase synthesis bank of a complex64 / complex128 CUDA tensor of shape (..., frames, bins) on the current stream, the
    mirror of pfb_channelize: bins = `channels`, or channels // 2 + 1 with real_output=True (explicit: the bins cannot tell the two
    kinds apart at channels <= 2); `filter` holds channels * taps reals of the same precision on the same device, shape
    (channels * taps,) or (taps, channels), or is None for all ones of one tap.  Returns (..., length) float (real_output) or complex,
    or `out`; length=None means (frames - 1) * hop + channels * taps.  Leading dimensions fold into the batch.  Handles are cached per
    (channels, taps, hop, dtype, kind, device) and the filter is set on EVERY call; keep an Ipfb to reuse one."""
    if not (_is_torch(Y) and Y.is_cuda and _precision(Y.dtype) is not None and not _precision(Y.dtype)[1]):
        raise TypeError("expected a CUDA complex64 / complex128 tensor")
    real = _precision(Y.dtype)[0]
    channels = int(channels)
    if channels < 1:
        raise ValueError(f"need channels >= 1, got {channels}")
    bins = channels // 2 + 1 if real_output else channels
    if Y.dim() < 2 or int(Y.shape[-1]) != bins:
        raise ValueError(f"expected (..., frames, {bins}) for {channels} channels, real_output={bool(real_output)}, got {tuple(Y.shape)}")
    taps = 1
    if filter is not None:
        if not (_is_torch(filter) and filter.is_cuda and filter.dtype == _torch_dtypes(real)[0] and filter.device == Y.device):
            raise TypeError(f"filter must be a CUDA {_names((_torch_dtypes(real)[0],))} tensor on the input's device")
        if filter.numel() == 0 or filter.numel() % channels or (filter.dim() == 2 and filter.shape[1] != channels) or filter.dim() not in (1, 2):
            raise ValueError(f"filter must hold channels * taps values as (channels * taps,) or (taps, {channels}), got {tuple(filter.shape)}")
        taps = filter.numel() // channels
        filter = filter.contiguous()
    p = _cached_plan(Ipfb, channels, taps, real, channels if hop is None else int(hop), bool(real_output), int(_device_index(Y)))
    p.set_filter(filter)
    return p.inverse(Y.contiguous(), length, out)


def pfb_reconstruction_terms(h, g, channels, hop):
    """What an analysis filter h and a synthesis filter g (channels * taps reals each, any shape) make of a signal that goes through
    Pfb and Ipfb, in the interior where every covering frame exists: y[t] = sum_{|s| < T} c_s(t mod D) x[t + s P] with
    c_s(r) = sum_j g[r + j D] h[r + j D + s P] over the j that keep both indices inside [0, P T).  Host-side numpy in float64; returns
    c of shape (2 T - 1, D), row s + T - 1 holding c_s.  Perfect reconstruction with zero delay: row T - 1 all ones, every other row zero."""
    P, D = int(channels), int(hop)
    hv = np.asarray(h.cpu() if _is_torch(h) else h, dtype=np.float64).reshape(-1)
    gv = np.asarray(g.cpu() if _is_torch(g) else g, dtype=np.float64).reshape(-1)
    if P < 1 or D < 1:
        raise ValueError(f"need channels >= 1 and hop >= 1, got {channels}, {hop}")
    if hv.size == 0 or hv.size % P or gv.size != hv.size:
        raise ValueError(f"h and g must hold the same multiple of {P} values, got {hv.size} and {gv.size}")
    span = hv.size
    T = span // P
    c = np.zeros((2 * T - 1, D))
    for s in range(-(T - 1), T):
        lo, hi = max(0, -s * P), min(span, span - s * P)  # the m with m and m + s P inside [0, P T)
        m = np.arange(lo, hi)
        np.add.at(c[s + T - 1], m % D, gv[m] * hv[m + s * P])
    return c


def pfb_prototype(channels, taps, dtype=None):
    """The usual windowed-sinc prototype filter of a `channels`-channel bank with `taps` taps: sinc((n - (P T - 1) / 2) / P) *
    hamming(P T)[n], n < P T, computed in float64 and rounded to `dtype` (a numpy dtype: a numpy array; a torch dtype: a CPU tensor;
    default numpy float64)."""
    P, T = int(channels), int(taps)
    if P < 1 or T < 1:
        raise ValueError(f"need channels >= 1 and taps >= 1, got {channels}, {taps}")
    n = np.arange(P * T, dtype=np.float64)
    h = np.sinc((n - (P * T - 1) / 2.0) / P) * np.hamming(P * T)
    if dtype is not None and type(dtype).__module__.startswith("torch"):
        import torch

        return torch.from_numpy(h).to(dtype)
    return h.astype(np.float64 if dtype is None else dtype)


class Mdct(_Handle):
    """Batched modified discrete cosine transform and its inverse (include/fourier.h, fourier_hip_mdct_*) on device memory: rows of
    `length` reals <-> frames x n reals per row, FRAME-MAJOR (frame f of row b at element offset (b * frames + f) * n).  A frame is 2n
    samples, the hop n; `center` pads n zeros in front and zeros behind by index arithmetic.  The window is set afterwards (set_window;
    default the sine window).  No envelope division: the inverse reconstructs where the window satisfies Princen-Bradley."""

    _prefix = "fourier_hip_mdct_"
    _destroy = "fourier_hip_mdct_destroy"

    def __init__(self, n, real="f32", center=True, device=-1):
        n = int(n)
        if n < 1:
            raise ValueError(f"need n >= 1, got {n}")
        self.center = bool(center)
        self._create(real, f"MDCT plan of {n} coefficients per frame, center {self.center}", n, int(self.center), int(device))
        self._n = n

    def size(self):
        return self._n

    def frames(self, length):
        """Frames of a row of `length` reals; 0 where the length is invalid."""
        return int(self._fn("frames")(self._h, int(length)))

    def default_length(self, frames):
        """The longest row `frames` frames give back: (frames - 1) n with center, (frames + 1) n without."""
        return (int(frames) - 1) * self._n if self.center else (int(frames) + 1) * self._n

    def set_option(self, key, value):
        """"fusion": 0 = the composed forward route, 1 = the fused one-launch route wherever it exists."""
        self._call("set_option", key.encode(), int(value), message=f"bad option {key}={value}")

    def reserve(self, length, batch):
        """Later forward calls of at most `batch` rows of `length` reals, and inverse calls to that length from frames(length) frames,
        never allocate."""
        self._call("reserve", int(length), int(batch))

    def set_window_ptr(self, d_window, stream=0):
        """2n reals of the handle's precision at d_window (0 / None: the sine window).  Waits for `stream`."""
        self._call("set_window", d_window or None, stream)

    def forward_ptr(self, d_in, d_out, length, batch, normalized=False, stream=0):
        """`batch` rows of `length` reals at d_in -> batch x frames(length) x n reals at d_out, enqueued on `stream`."""
        self._call("forward", d_in, d_out, int(length), int(batch), int(bool(normalized)), stream)

    def inverse_ptr(self, d_in, d_out, frames, length, batch, normalized=False, stream=0):
        """batch x frames x n reals at d_in -> `batch` rows of `length` reals at d_out, enqueued on `stream`."""
        self._call("inverse", d_in, d_out, int(frames), int(length), int(batch), int(bool(normalized)), stream)

    def set_window(self, window):
        """A contiguous CUDA tensor of 2n reals of the handle's precision, or None for the sine window; on the current stream."""
        if window is None:
            return self.set_window_ptr(None)
        _require_cuda(window, _torch_dtypes(self.real)[0])
        if tuple(window.shape) != (2 * self._n,):
            raise ValueError(f"window must have shape ({2 * self._n},), got {tuple(window.shape)}")
        self.set_window_ptr(window.data_ptr(), _stream(window))

    def forward(self, x, normalized=False, out=None):
        """Contiguous (..., length) real CUDA tensor -> a new (..., frames, n) real tensor (frame-major), or `out`, on the current
        stream."""
        import torch

        rdt = _torch_dtypes(self.real)[0]
        _require_cuda(x, rdt)
        if x.dim() == 0:
            raise ValueError("expected at least one dimension")
        length = int(x.shape[-1])
        fr = self.frames(length)
        if fr == 0:
            raise ValueError(f"a row of {length} samples is too short for n {self._n} with center {self.center}")
        shape = tuple(x.shape[:-1]) + (fr, self._n)
        if out is None:
            out = torch.empty(shape, dtype=rdt, device=x.device)
        else:
            _require_out(out, shape, rdt, x.device)
        batch = x.numel() // length
        if batch:
            self.forward_ptr(x.data_ptr(), out.data_ptr(), length, batch, normalized, _stream(x))
        return out

    def inverse(self, X, length=None, normalized=False, out=None):
        """Contiguous (..., frames, n) real CUDA tensor (frame-major) -> a new (..., length) real tensor, or `out`, on the current
        stream; length defaults to default_length(frames)."""
        import torch

        rdt = _torch_dtypes(self.real)[0]
        _require_cuda(X, rdt)
        if X.dim() < 2 or X.shape[-1] != self._n or X.shape[-2] == 0:
            raise ValueError(f"expected (..., frames >= 1, {self._n}), got {tuple(X.shape)}")
        fr = int(X.shape[-2])
        full = self.default_length(fr)
        length = full if length is None else int(length)
        if not 1 <= length <= full:
            raise ValueError(f"length must be in 1 ... {full} for {fr} frames, got {length}")
        shape = tuple(X.shape[:-2]) + (length,)
        if out is None:
            out = torch.empty(shape, dtype=rdt, device=X.device)
        else:
            _require_out(out, shape, rdt, X.device)
        batch = X.numel() // (fr * self._n)
        if batch:
            self.inverse_ptr(X.data_ptr(), out.data_ptr(), fr, length, batch, normalized, _stream(X))
        return out


def create_mdct_f32(n, center=True, device=-1):
    return Mdct(n, "f32", center, device)


def create_mdct_f64(n, center=True, device=-1):
    return Mdct(n, "f64", center, device)


def _mdct_plan(x, n, window, center):
    """The cached handle of these parameters with `window` set (on every call, like stft's)."""
    import torch

    if not (_is_torch(x) and x.is_cuda and x.dtype in (torch.float32, torch.float64)):
        raise TypeError("expected a CUDA float32 / float64 tensor")
    n = int(n)
    if n < 1:
        raise ValueError(f"need n >= 1, got {n}")
    real = _precision(x.dtype)[0]
    if window is not None:
        if not (_is_torch(window) and window.is_cuda and window.dtype == x.dtype and window.device == x.device):
            raise TypeError(f"window must be a CUDA {_names((x.dtype,))} tensor on the input's device")
        if tuple(window.shape) != (2 * n,):
            raise ValueError(f"window must have shape ({2 * n},), got {tuple(window.shape)}")
        window = window.contiguous()
    p = _cached_plan(Mdct, n, real, bool(center), int(_device_index(x)))
    p.set_window(window)
    return p


def mdct(x, n, window=None, center=True, normalized=False):
    """The MDCT of a float32 / float64 CUDA tensor of shape (..., length) on the current stream -> (..., frames, n), frames of 2n
    samples every n samples, `window` of 2n reals (None: the sine window), `center` pads n zeros in front and zeros behind; times
    sqrt(2 / n) where normalized.  Leading dimensions fold into the batch.  Handles are cached per (n, center, dtype, device) and the
    window is set on EVERY call; keep an Mdct to reuse one."""
    p = _mdct_plan(x, n, window, center)
    if x.dim() == 0:
        raise ValueError("expected at least one dimension")
    return p.forward(x.contiguous(), normalized)


def imdct(X, n, window=None, center=True, normalized=False, length=None):
    """The inverse MDCT with overlap-add of a float32 / float64 CUDA tensor of shape (..., frames, n) on the current stream ->
    (..., length) reals, length defaulting to (frames - 1) n with center and (frames + 1) n without.  No envelope division: it
    reconstructs mdct's input where the window satisfies Princen-Bradley (the sine default does)."""
    p = _mdct_plan(X, n, window, center)
    if X.dim() < 2:
        raise ValueError("expected shape (..., frames, n)")
    return p.inverse(X.contiguous(), length, normalized)


class RealFftN(_RealHandle):
    """Batched real-input N-D transforms (include/fourier.h, fourier_hip_realnd_*) over items of `shape` (1 ... 4 dimensions, the
    last one real) on device memory, numpy's rfftn / irfftn layout: an item of reals has `shape`, an item of the half spectrum has
    shape[:-1] + (shape[-1]//2+1,).  Forward codes Fft / SqrtScaledFft, inverse codes Ifft / UnscaledIfft / SqrtScaledIfft, scaled
    over the product of the lengths."""

    _prefix = "fourier_hip_realnd_"
    _destroy = "fourier_hip_realnd_destroy"

    def __init__(self, shape, real, device=-1):
        import ctypes

        self.shape = tuple(int(n) for n in shape)
        dims = (ctypes.c_size_t * max(1, len(self.shape)))(*self.shape)
        self._create(real, f"real N-D FFT plan of shape {self.shape}", len(self.shape), dims, int(device))

    def rank(self):
        return len(self.shape)

    def half_shape(self):
        return self.shape[:-1] + (self.shape[-1] // 2 + 1,)


def set_default_option(key, value):
    """Library-wide default for plans created afterwards (include/fourier.h: fourier_hip_set_default_option), e.g.
    ("specialise_at_create", 2): lengths whose prime factors stop at 13 get their own kernels compiled inside create_fft_*."""
    L = _lib.lib()
    _raise_status(L, L.fourier_hip_set_default_option(key.encode(), int(value)), f"bad default option {key}={value}")


def get_default_option(key):
    return int(_lib.lib().fourier_hip_get_default_option(key.encode()))


def create_fft_f32(size, device=-1):
    """fourier/src/lib.rs:31-43."""
    return Fft(size, "f32", device)


def create_fft_f64(size, device=-1):
    """fourier/src/lib.rs:49-60."""
    return Fft(size, "f64", device)


def fftn(x, dims=None, transform=Transform.Fft, out=None):
    """N-dimensional transform of a contiguous CUDA complex64 / complex128 tensor over `dims` (default: all), one axis transform per
    dimension on the current stream.  Returns a new tensor, or `out` (which may be `x`).  Scaling per axis as numpy: Ifft is ifftn,
    the sqrt-scaled codes are norm="ortho"."""
    import torch

    _require_cuda(x, _torch_dtypes("f32")[1], _torch_dtypes("f64")[1])
    transform = Transform(transform)
    norm = _normalise_dims(x.dim(), dims)
    if out is None:
        out = torch.empty_like(x)
    elif out is not x:
        _require_out(out, x.shape, x.dtype, x.device)
    real, device = _precision(x.dtype)[0], int(_device_index(x))
    src = x
    for d in norm:
        if x.shape[d] == 1:  # a 1-point transform is the identity under every code
            continue
        _cached_plan(Fft, int(x.shape[d]), real, device).transform_axis(src, out, transform, d)
        src = out
    if src is x and out is not x:  # every axis skipped
        out.copy_(x)
    return out


def fft2(x, transform=Transform.Fft, out=None):
    """fftn over the last two dimensions."""
    return fftn(x, (-2, -1), transform, out)


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
    norm = _normalise_dims(ndim, dims)
    k = len(norm)
    if sorted(norm) == list(range(ndim - k, ndim)) and norm[-1] == ndim - 1:
        return norm, None
    batch = [d for d in range(ndim) if d not in norm]
    return norm, tuple(batch + sorted(norm[:-1]) + [norm[-1]])


def _realnd_run(x, dims, shape_of, forward, transform, out):
    """rfftn / irfftn behind the layout rule of realnd_layout: the plan of the transformed shape over the batch in front."""
    import torch

    real = _precision(x.dtype)[0]
    out_dtype = _torch_dtypes(real)[1 if forward else 0]
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
    if out is not None:
        _require_out(out, want, out_dtype, x.device)
    res = out if (out is not None and perm is None) else torch.empty(res_shape, dtype=out_dtype, device=x.device)
    items = 1
    for n in src.shape[:src.dim() - k]:
        items *= n
    plan = _cached_plan(RealFftN, tuple(int(n) for n in shape), real, int(_device_index(x)))
    if items:
        run = plan.forward_batch_ptr if forward else plan.inverse_batch_ptr
        run(src.data_ptr(), res.data_ptr(), items, transform, _stream(x))
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
    _require_cuda(x, _torch_dtypes("f32")[0], _torch_dtypes("f64")[0])
    transform = Transform(transform)
    if not transform.is_forward():
        raise ValueError(f"{transform!r} is not a forward transform")
    return _realnd_run(x, dims, lambda s: s, True, transform, out)


def irfftn(X, dims=None, n=None, transform=Transform.Ifft, out=None):
    """Inverse of rfftn: a contiguous CUDA complex64 / complex128 half spectrum over `dims` (the last entry is the half-spectrum axis)
    -> reals, `n` (default 2 * (X.shape[last] - 1)) on the real axis, on the current stream.  numpy's irfftn scaling: Ifft is the
    default, SqrtScaledIfft is norm="ortho", UnscaledIfft is norm="forward".  Input that is not Hermitian gives numpy's result.
    X is not modified."""
    _require_cuda(X, _torch_dtypes("f32")[1], _torch_dtypes("f64")[1])
    transform = Transform(transform)
    if transform.is_forward():
        raise ValueError(f"{transform!r} is not an inverse transform")

    def shape_of(s):
        m = 2 * (s[-1] - 1) if n is None else int(n)
        if m < 1 or m // 2 + 1 != s[-1]:
            raise ValueError(f"real length {m} does not match {s[-1]} half-spectrum values")
        return s[:-1] + (m,)

    return _realnd_run(X, dims, shape_of, False, transform, out)


def rfft2(x, transform=Transform.Fft, out=None):
    """rfftn over the last two dimensions."""
    return rfftn(x, (-2, -1), transform, out)


def irfft2(X, n=None, transform=Transform.Ifft, out=None):
    """irfftn over the last two dimensions."""
    return irfftn(X, (-2, -1), n, transform, out)
