"""ctypes binding of the C ABI declared in include/fourier.h (libfourier.so).

There is deliberately no CPU fallback: if the HIP library has not been built, importing the
operator layer raises.  (The reference's FFI, fourier-ffi/src/lib.rs:14-106, is bound the other way
round; see INTEGRATION.md for the Rust shim.)
"""
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libfourier.so")

SUFFIXES = ("float", "double")

vp, sz, ci, ll, cp = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_longlong, ctypes.c_char_p
_BATCH = (ci, [vp, vp, vp, sz, ci, vp])  # handle, d_in, d_out, batch, code, stream

# Every entry point include/fourier.h declares, written once: (prefix, {symbol stem: (restype, argtypes)}) per handle family.  A symbol
# is <prefix><stem>_<float|double>; the lists of names below and bind() are both derived from these tables.
_LEGACY = ("fourier_", {  # the reference's FFI
    "create": (vp, [sz]), "destroy": (None, [vp]), "transform_in_place": (None, [vp, vp, ci]), "transform": (None, [vp, vp, vp, ci])})
_EXT = ("fourier_hip_", {  # the complex handle's extensions
    "create": (vp, [sz, ci]), "size": (sz, [vp]), "transform_batch": _BATCH, "reserve": (ci, [vp, sz, ci]), "device": (ci, [vp]),
    "synchronize": (ci, [vp, vp]), "transform_batch_host": (ci, [vp, vp, vp, sz, ci]), "last_status": (ci, [vp]),
    "set_option": (ci, [vp, cp, ll]), "describe": (cp, [vp]), "model_bytes": (ctypes.c_double, [vp]),
    "profile": (ci, [vp, vp, vp, sz, ci, vp, ci, ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ci)]), "slot_names": (cp, [vp])})
_REAL = ("fourier_hip_real_", {  # real-input transforms
    "create": (vp, [sz, ci]), "destroy": (None, [vp]), "size": (sz, [vp]), "forward_batch": _BATCH, "inverse_batch": _BATCH,
    "reserve": (ci, [vp, sz]), "describe": (cp, [vp]), "last_status": (ci, [vp])})
_AXIS = ("fourier_hip_", {  # transforms along a strided axis (methods of the complex handle)
    "transform_axis": (ci, [vp, vp, vp, sz, sz, ci, vp]), "reserve_axis": (ci, [vp, sz, sz]), "describe_axis": (cp, [vp, sz])})
_REALND = ("fourier_hip_realnd_", {  # real-input N-D transforms
    "create": (vp, [ci, ctypes.POINTER(sz), ci]), "destroy": (None, [vp]), "rank": (ci, [vp]), "forward_batch": _BATCH,
    "inverse_batch": _BATCH, "reserve": (ci, [vp, sz]), "describe": (cp, [vp]), "last_status": (ci, [vp])})
_CONV = ("fourier_hip_conv_", {  # convolution with a prepared filter bank
    "create": (vp, [sz, ci, ci]), "destroy": (None, [vp]), "size": (sz, [vp]), "filters": (sz, [vp]),
    "set_filters": (ci, [vp, vp, sz, sz, ci, vp]), "apply": (ci, [vp, vp, vp, sz, vp]), "reserve": (ci, [vp, sz]),
    "set_option": (ci, [vp, cp, ll]), "describe": (cp, [vp]), "last_status": (ci, [vp])})
_CONVND = ("fourier_hip_convnd_", {  # N-D convolution of real items with a prepared filter bank
    "create": (vp, [ci, ctypes.POINTER(sz), ci]), "destroy": (None, [vp]), "rank": (ci, [vp]), "shape": (ci, [vp, ctypes.POINTER(sz)]),
    "filters": (sz, [vp]),
    "set_filters": (ci, [vp, vp, ctypes.POINTER(sz), sz, ci, vp]),  # handle, d_taps, taps_shape, filters, correlate, stream
    "set_window": (ci, [vp, ctypes.POINTER(sz), ctypes.POINTER(sz), ctypes.POINTER(sz)]),  # handle, in_shape, out_first, out_shape
    "apply_batch": (ci, [vp, vp, vp, sz, sz, vp]),  # handle, d_in, d_out, batch, filter_first, stream
    "reserve": (ci, [vp, sz]), "set_option": (ci, [vp, cp, ll]), "describe": (cp, [vp]), "last_status": (ci, [vp])})
_LCONV = ("fourier_hip_lconv_", {  # linear convolution (full / same / valid) with a prepared filter bank
    "create": (vp, [sz, sz, ci, ci, ci]), "destroy": (None, [vp]), "length": (sz, [vp]), "taps": (sz, [vp]), "out_length": (sz, [vp]),
    "filters": (sz, [vp]), "set_filters": (ci, [vp, vp, sz, ci, vp]), "apply": (ci, [vp, vp, vp, sz, vp]), "reserve": (ci, [vp, sz]),
    "set_option": (ci, [vp, cp, ll]), "describe": (cp, [vp]), "last_status": (ci, [vp])})
_R2R = ("fourier_hip_r2r_", {  # DCT / DST of types II and III
    "create": (vp, [sz, ci]), "destroy": (None, [vp]), "size": (sz, [vp]),
    "transform_batch": (ci, [vp, vp, vp, sz, ci, ci, vp]),  # handle, d_in, d_out, batch, kind, norm, stream
    "reserve": (ci, [vp, sz]), "describe": (cp, [vp]), "last_status": (ci, [vp])})
_STFT = ("fourier_hip_stft_", {  # short-time Fourier transform and its inverse
    "create": (vp, [sz, sz, sz, ci, ci]), "destroy": (None, [vp]), "n_fft": (sz, [vp]), "hop": (sz, [vp]), "win_length": (sz, [vp]),
    "bins": (sz, [vp]), "frames": (sz, [vp, sz]), "set_window": (ci, [vp, vp, vp]),
    "forward": (ci, [vp, vp, vp, sz, sz, ci, vp]),      # handle, d_in, d_out, length, batch, normalized, stream
    "inverse": (ci, [vp, vp, vp, sz, sz, sz, ci, vp]),  # handle, d_in, d_out, frames, length, batch, normalized, stream
    "reserve": (ci, [vp, sz, sz]), "set_option": (ci, [vp, cp, ll]), "describe": (cp, [vp]), "last_status": (ci, [vp])})
_MDCT = ("fourier_hip_mdct_", {  # modified discrete cosine transform and its inverse
    "create": (vp, [sz, ci, ci]), "destroy": (None, [vp]), "size": (sz, [vp]), "frames": (sz, [vp, sz]), "set_window": (ci, [vp, vp, vp]),
    "forward": (ci, [vp, vp, vp, sz, sz, ci, vp]),      # handle, d_in, d_out, length, batch, normalized, stream
    "inverse": (ci, [vp, vp, vp, sz, sz, sz, ci, vp]),  # handle, d_in, d_out, frames, length, batch, normalized, stream
    "reserve": (ci, [vp, sz, sz]), "set_option": (ci, [vp, cp, ll]), "describe": (cp, [vp]), "last_status": (ci, [vp])})
_SPECTROGRAM = ("fourier_hip_spectrogram_", {  # power spectrogram and Welch average on the STFT's frames
    "create": (vp, [sz, sz, sz, ci, ci]), "destroy": (None, [vp]), "n_fft": (sz, [vp]), "hop": (sz, [vp]), "win_length": (sz, [vp]),
    "bins": (sz, [vp]), "frames": (sz, [vp, sz]), "set_window": (ci, [vp, vp, vp]),
    "forward": (ci, [vp, vp, vp, sz, sz, ci, ci, vp]),           # handle, d_in, d_out, length, batch, power, normalized, stream
    "welch": (ci, [vp, vp, vp, sz, sz, ci, ctypes.c_double, vp]),  # handle, d_in, d_out, length, batch, onesided_fold, scale, stream
    "reserve": (ci, [vp, sz, sz]), "set_option": (ci, [vp, cp, ll]), "describe": (cp, [vp]), "last_status": (ci, [vp])})
_CSD = ("fourier_hip_csd_", {  # cross-spectral density and coherence of two signals on the STFT's frames
    "create": (vp, [sz, sz, sz, ci, ci]), "destroy": (None, [vp]), "n_fft": (sz, [vp]), "hop": (sz, [vp]), "win_length": (sz, [vp]),
    "bins": (sz, [vp]), "frames": (sz, [vp, sz]), "set_window": (ci, [vp, vp, vp]),
    "csd": (ci, [vp, vp, vp, vp, sz, sz, ci, ctypes.c_double, vp]),  # handle, d_x, d_y, d_out, length, batch, onesided_fold, scale, stream
    "coherence": (ci, [vp, vp, vp, vp, sz, sz, vp]),                 # handle, d_x, d_y, d_out, length, batch, stream
    "reserve": (ci, [vp, sz, sz]), "set_option": (ci, [vp, cp, ll]), "describe": (cp, [vp]), "last_status": (ci, [vp])})
_BANDSPEC = ("fourier_hip_bandspec_", {  # band-energy (mel) spectrogram: a sparse-row projection of |X|^p on the STFT's frames
    "create": (vp, [sz, sz, sz, ci, sz, ci]),  # n_fft, hop, win_length, pad_mode, bands, device
    "destroy": (None, [vp]), "n_fft": (sz, [vp]), "hop": (sz, [vp]), "win_length": (sz, [vp]), "bins": (sz, [vp]), "bands": (sz, [vp]),
    "frames": (sz, [vp, sz]), "set_window": (ci, [vp, vp, vp]),
    "set_bands": (ci, [vp, vp, vp]),  # handle, h_matrix (HOST, bands x bins reals), stream
    "forward": (ci, [vp, vp, vp, sz, sz, ci, ci, ctypes.c_double, ctypes.c_double, vp]),  # handle, d_in, d_out, length, batch, power, normalized, log_mult, log_floor, stream
    "reserve": (ci, [vp, sz, sz]), "set_option": (ci, [vp, cp, ll]), "describe": (cp, [vp]), "last_status": (ci, [vp])})
_HILBERT = ("fourier_hip_hilbert_", {  # analytic signal and envelope of real rows
    "create": (vp, [sz, ci]), "destroy": (None, [vp]), "size": (sz, [vp]),
    "analytic": (ci, [vp, vp, vp, sz, vp]), "envelope": (ci, [vp, vp, vp, sz, vp]),  # handle, d_in, d_out, batch, stream
    "reserve": (ci, [vp, sz]), "set_option": (ci, [vp, cp, ll]), "describe": (cp, [vp]), "last_status": (ci, [vp])})
_CZT = ("fourier_hip_czt_", {  # chirp-z transform: n samples in, m points of a z-plane arc or spiral out
    "create": (vp, [sz, sz, ctypes.c_double, ctypes.c_double, ctypes.c_double, ctypes.c_double, ci, ci]),  # n, m, w_abs, w_turns, a_abs, a_turns, real_input, device
    "destroy": (None, [vp]), "size": (sz, [vp]), "points": (sz, [vp]),
    "transform": (ci, [vp, vp, vp, sz, vp]),  # handle, d_in, d_out, batch, stream
    "reserve": (ci, [vp, sz]), "set_option": (ci, [vp, cp, ll]), "describe": (cp, [vp]), "last_status": (ci, [vp])})
_PFB = ("fourier_hip_pfb_", {  # polyphase filter bank channelizer
    "create": (vp, [sz, sz, sz, ci, ci]),  # channels, taps, hop, real_input, device
    "destroy": (None, [vp]), "channels": (sz, [vp]), "taps": (sz, [vp]), "hop": (sz, [vp]), "bins": (sz, [vp]), "frames": (sz, [vp, sz]),
    "set_filter": (ci, [vp, vp, vp]),
    "forward": (ci, [vp, vp, vp, sz, sz, vp]),  # handle, d_in, d_out, length, batch, stream
    "reserve": (ci, [vp, sz, sz]), "set_option": (ci, [vp, cp, ll]), "describe": (cp, [vp]), "last_status": (ci, [vp])})
_IPFB = ("fourier_hip_ipfb_", {  # polyphase synthesis filter bank
    "create": (vp, [sz, sz, sz, ci, ci]),  # channels, taps, hop, real_output, device
    "destroy": (None, [vp]), "channels": (sz, [vp]), "taps": (sz, [vp]), "hop": (sz, [vp]), "bins": (sz, [vp]), "length": (sz, [vp, sz]),
    "set_filter": (ci, [vp, vp, vp]),
    "inverse": (ci, [vp, vp, vp, sz, sz, sz, vp]),  # handle, d_in, d_out, frames, length, batch, stream
    "reserve": (ci, [vp, sz, sz]), "describe": (cp, [vp]), "last_status": (ci, [vp])})
_RESAMPLE = ("fourier_hip_resample_", {  # Fourier-domain resampling of complex or real rows
    "create": (vp, [sz, sz, ci, ci]),  # n_in, n_out, real_input, device
    "destroy": (None, [vp]), "size_in": (sz, [vp]), "size_out": (sz, [vp]), "real_input": (ci, [vp]),
    "forward": (ci, [vp, vp, vp, sz, vp]),  # handle, d_in, d_out, batch, stream
    "set_window": (ci, [vp, vp, vp]),
    "reserve": (ci, [vp, sz]), "set_option": (ci, [vp, cp, ll]), "describe": (cp, [vp]), "last_status": (ci, [vp])})
_XCORR = ("fourier_hip_xcorr_", {  # pairwise cross-correlation and GCC-PHAT of real or complex rows
    "create": (vp, [sz, sz, ll, sz, ci, ci]),  # size, length, lag_first, lags, real_data, device
    "destroy": (None, [vp]), "size": (sz, [vp]), "length": (sz, [vp]), "lags": (sz, [vp]),
    "correlate": (ci, [vp, vp, vp, vp, sz, vp]),  # handle, d_x, d_y, d_out, batch, stream
    "reserve": (ci, [vp, sz]), "set_option": (ci, [vp, cp, ll]), "describe": (cp, [vp]), "last_status": (ci, [vp])})
_DELAY = ("fourier_hip_delay_", {  # fractional delay and delay-and-sum of real or complex rows, delays and weights on the device
    "create": (vp, [sz, sz, sz, ci, ci]),  # size, length, channels, real_data, device
    "destroy": (None, [vp]), "size": (sz, [vp]), "length": (sz, [vp]), "channels": (sz, [vp]),
    "apply": (ci, [vp, vp, vp, vp, vp, sz, vp]),  # handle, d_in, d_delays, d_weights (may be NULL), d_out, batch, stream
    "reserve": (ci, [vp, sz]), "set_option": (ci, [vp, cp, ll]), "describe": (cp, [vp]), "last_status": (ci, [vp])})
_CEPSTRUM = ("fourier_hip_cepstrum_", {  # real cepstrum (mode 0) and minimum-phase reconstruction (mode 1) of real rows
    "create": (vp, [sz, sz, sz, ci, ci]),  # size, length, outputs, mode, device
    "destroy": (None, [vp]), "size": (sz, [vp]), "length": (sz, [vp]), "outputs": (sz, [vp]), "mode": (ci, [vp]),
    "apply": (ci, [vp, vp, vp, sz, ctypes.c_double, ctypes.c_double, vp]),  # handle, d_in, d_out, batch, log_mult, log_floor, stream
    "reserve": (ci, [vp, sz]), "set_option": (ci, [vp, cp, ll]), "describe": (cp, [vp]), "last_status": (ci, [vp])})
_NUFFT = ("fourier_hip_nufft_", {  # non-uniform FFT, 1-D types 1 and 2, points shared by the rows of a batch
    "create": (vp, [sz, ctypes.c_double, ci]),  # n_modes, eps, device
    "destroy": (None, [vp]), "modes": (sz, [vp]), "points": (sz, [vp]),
    "set_points": (ci, [vp, vp, sz, vp]),  # handle, h_points (f64 on the host), m, stream
    "to_modes_batch": (ci, [vp, vp, vp, sz, ci, ci, vp]),  # handle, d_in, d_out, batch, sign, order, stream
    "to_points_batch": (ci, [vp, vp, vp, sz, ci, ci, vp]),
    "reserve": (ci, [vp, sz]), "set_option": (ci, [vp, cp, ll]), "describe": (cp, [vp]), "last_status": (ci, [vp])})
_NUFFT2D = ("fourier_hip_nufft2d_", {  # non-uniform FFT, 2-D types 1 and 2, points shared by the items of a batch
    "create": (vp, [sz, sz, ctypes.c_double, ci]),  # n1, n2, eps, device
    "destroy": (None, [vp]), "modes1": (sz, [vp]), "modes2": (sz, [vp]), "points": (sz, [vp]),
    "set_points": (ci, [vp, vp, vp, sz, vp]),  # handle, h_x1, h_x2 (f64 on the host), m, stream
    "to_modes_batch": (ci, [vp, vp, vp, sz, ci, ci, vp]),  # handle, d_in, d_out, batch, sign, order, stream
    "to_points_batch": (ci, [vp, vp, vp, sz, ci, ci, vp]),
    "reserve": (ci, [vp, sz]), "set_option": (ci, [vp, cp, ll]), "describe": (cp, [vp]), "last_status": (ci, [vp])})
_NUFFT3D = ("fourier_hip_nufft3d_", {  # non-uniform FFT, 3-D types 1 and 2, points shared by the items of a batch
    "create": (vp, [sz, sz, sz, ctypes.c_double, ci]),  # n1, n2, n3, eps, device
    "destroy": (None, [vp]), "modes1": (sz, [vp]), "modes2": (sz, [vp]), "modes3": (sz, [vp]), "points": (sz, [vp]),
    "set_points": (ci, [vp, vp, vp, vp, sz, vp]),  # handle, h_x1, h_x2, h_x3 (f64 on the host), m, stream
    "to_modes_batch": (ci, [vp, vp, vp, sz, ci, ci, vp]),  # handle, d_in, d_out, batch, sign, order, stream
    "to_points_batch": (ci, [vp, vp, vp, sz, ci, ci, vp]),
    "reserve": (ci, [vp, sz]), "set_option": (ci, [vp, cp, ll]), "describe": (cp, [vp]), "last_status": (ci, [vp])})
_GLOBAL = {  # no handle, no precision suffix
    "fourier_hip_status_string": (cp, [ci]), "fourier_hip_set_default_option": (ci, [cp, ll]),
    "fourier_hip_get_default_option": (ll, [cp])}


def _signatures(family):
    prefix, table = family
    return {f"{prefix}{op}_{s}": table[op] for s in SUFFIXES for op in table}


LEGACY_SYMBOLS = list(_signatures(_LEGACY))
EXT_SYMBOLS = list(_signatures(_EXT)) + list(_GLOBAL)
REAL_SYMBOLS = list(_signatures(_REAL))
AXIS_SYMBOLS = list(_signatures(_AXIS))
REALND_SYMBOLS = list(_signatures(_REALND))
CONV_SYMBOLS = list(_signatures(_CONV))
LCONV_SYMBOLS = list(_signatures(_LCONV))
STFT_SYMBOLS = list(_signatures(_STFT))
MDCT_SYMBOLS = list(_signatures(_MDCT))
SPECTROGRAM_SYMBOLS = list(_signatures(_SPECTROGRAM))
CSD_SYMBOLS = list(_signatures(_CSD))
BANDSPEC_SYMBOLS = list(_signatures(_BANDSPEC))
HILBERT_SYMBOLS = list(_signatures(_HILBERT))
CZT_SYMBOLS = list(_signatures(_CZT))
PFB_SYMBOLS = list(_signatures(_PFB))
IPFB_SYMBOLS = list(_signatures(_IPFB))
RESAMPLE_SYMBOLS = list(_signatures(_RESAMPLE))
XCORR_SYMBOLS = list(_signatures(_XCORR))
DELAY_SYMBOLS = list(_signatures(_DELAY))
CEPSTRUM_SYMBOLS = list(_signatures(_CEPSTRUM))
CONVND_SYMBOLS = list(_signatures(_CONVND))
NUFFT_SYMBOLS = list(_signatures(_NUFFT))
ALL_SYMBOLS = (LEGACY_SYMBOLS + EXT_SYMBOLS + REAL_SYMBOLS + AXIS_SYMBOLS + REALND_SYMBOLS + CONV_SYMBOLS + LCONV_SYMBOLS + STFT_SYMBOLS + MDCT_SYMBOLS
               + SPECTROGRAM_SYMBOLS + CSD_SYMBOLS + BANDSPEC_SYMBOLS + HILBERT_SYMBOLS + CZT_SYMBOLS + PFB_SYMBOLS + IPFB_SYMBOLS + RESAMPLE_SYMBOLS + XCORR_SYMBOLS + DELAY_SYMBOLS + CEPSTRUM_SYMBOLS + CONVND_SYMBOLS + NUFFT_SYMBOLS)
# The r2r family is listed apart: tests/test_abi.py compares ALL_SYMBOLS with the names a letters-only pattern finds in the header,
# and that pattern cannot see a name with a digit in it.  tests/test_r2r_abi.py holds the same three-way check for these.
R2R_SYMBOLS = list(_signatures(_R2R))
# ... and so is the 2-D non-uniform FFT family, for the digit in "nufft2d": tests/test_nufft2d_abi.py holds its three-way check.
NUFFT2D_SYMBOLS = list(_signatures(_NUFFT2D))
# ... and the 3-D one, for the same reason: tests/test_nufft3d_abi.py.
NUFFT3D_SYMBOLS = list(_signatures(_NUFFT3D))


def bind(cdll, strict=True):
    """Attach argtypes/restypes for every entry point of include/fourier.h to a loaded CDLL.  strict=False (A/B tools that
    load libraries built from older sources) tolerates entry points added since."""
    signatures = dict(_GLOBAL)
    for family in (_LEGACY, _EXT, _REAL, _AXIS, _REALND, _CONV, _LCONV, _R2R, _STFT, _MDCT, _SPECTROGRAM, _CSD, _BANDSPEC, _HILBERT, _CZT, _PFB, _IPFB, _RESAMPLE, _XCORR, _DELAY, _CEPSTRUM, _CONVND, _NUFFT, _NUFFT2D, _NUFFT3D):
        signatures.update(_signatures(family))
    for name, (restype, argtypes) in signatures.items():
        if strict or hasattr(cdll, name):
            f = getattr(cdll, name)
            f.restype, f.argtypes = restype, argtypes
    return cdll


_lib = None


def lib():
    """The product library.  Raises if the HIP build is missing (no fallback by design)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(
                f"{LIB_PATH} not found: build the HIP engine first "
                "(python -c 'import __graft_entry__ as g; g.build()' or python -m fourier_amd.build)")
        try:  # when torch is around, load it first so both share one HIP runtime (same SONAME)
            import torch  # noqa: F401
        except Exception:
            pass
        _lib = bind(ctypes.CDLL(LIB_PATH))
    return _lib
