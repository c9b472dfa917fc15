"""fourier_amd: MI355X-native batched 1D c2c FFT engine behind calebzulawski/fourier's plan API.

Only the hot path lives here: csrc/ (HIP kernels + the C ABI of include/fourier.h) and the host-side
mirror of the reference's operator interface (fft.py).
"""
from .fft import (R2R, CrossSpectrum, Fft, FftConv, FourierError, Hilbert, LinearConv, Mdct, RealFft, RealFftN, Spectrogram, Stft, Transform, create_conv_f32, create_conv_f64, create_csd_f32, create_csd_f64, create_fft_f32,  # noqa: F401
                  create_fft_f64, create_lconv_f32, create_lconv_f64, create_mdct_f32, create_mdct_f64, create_r2r_f32, create_r2r_f64, create_rfft_f32, create_rfft_f64, create_spectrogram_f32, create_spectrogram_f64, create_stft_f32, create_stft_f64, dct, dst, fft2, fftconv, fftconvolve, fftn, get_default_option, idct, idst, imdct,
                  irfft2, irfftn, istft, mdct, realnd_layout, rfft2, rfftn, set_default_option, spectrogram, stft, welch, coherence, csd, create_hilbert_f32, create_hilbert_f64, envelope, hilbert, Czt, create_czt_f32, create_czt_f64, czt, zoom_fft, Pfb, create_pfb_f32, create_pfb_f64, pfb_channelize, pfb_prototype, Ipfb, create_ipfb_f32, create_ipfb_f64, pfb_synthesize, pfb_reconstruction_terms, Resample, create_resample_f32, create_resample_f64, resample, BandSpectrogram, create_bandspec_f32, create_bandspec_f64, band_spectrogram, mel_filterbank, mel_spectrogram, mfcc, CrossCorrelation, create_xcorr_f32, create_xcorr_f64, xcorr, gcc_phat, correlation_lags, Delay, create_delay_f32, create_delay_f64, fractional_delay, delay_and_sum)
