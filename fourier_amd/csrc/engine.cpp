// engine.cpp -- host side of libfourier.so: plan factory, pass scheduling, C ABI.
//
// Mirrors the reference's plan layer one level up:
//   create_fft_f32/f64  (fourier/src/lib.rs:31-60)        -> Plan<T>::create      (Stockham, else Bluestein)
//   Autosort::new       (autosort/mod.rs:104-134)         -> Pow2Engine<T>        (big-radix pass schedule)
//   initialize_twiddles (autosort/mod.rs:24-46)           -> make_stage_tables / make_two_level (f64 trig, cast)
//   Bluesteins::new     (bluesteins.rs:109-130, :18-61)   -> Plan<T>::init_bluestein
//   apply_stages / apply (mod.rs:313-404, bluesteins.rs:215-259) -> Plan<T>::exec
//   fourier-ffi C ABI   (fourier-ffi/src/lib.rs:14-106)   -> extern "C" block at the end
// This translation unit holds the host logic only (engine_pow2.h, engine_mixed.h, engine_generic.h, plan.h) and the C
// ABI; the kernels are instantiated in kernels_*.cpp, one object per family and precision, and reached through the registry
// of engine_common.h.  Compiled with hipcc for gfx950; the same files build against tests/emu/hipemu.h (-DFOURIER_EMU)
// for CPU-side logic tests only.
#include "plan.h"
#include "real_plan.h"
#include "axis_plan.h"
#include "realnd_plan.h"
#include "conv_plan.h"
#include "convnd_plan.h"
#include "lconv_plan.h"
#include "r2r_plan.h"
#include "stft_plan.h"
#include "mdct_plan.h"
#include "spectrogram_plan.h"
#include "csd_plan.h"
#include "bandspec_plan.h"
#include "hilbert_plan.h"
#include "czt_plan.h"
#include "pfb_plan.h"
#include "ipfb_plan.h"
#include "resample_plan.h"
#include "xcorr_plan.h"
#include "delay_plan.h"
#include "cepstrum_plan.h"
#include "nufft_plan.h"
#include "nufft2d_plan.h"
#include "nufft3d_plan.h"

// ---------------------------------------------------------------------------------------------
// C ABI (declared in include/fourier.h)
using namespace fourier_hip;
namespace fc = ::fourier::c;

// what every handle family's entry points do in the same way; H = the handle class behind the opaque pointer
template <typename H> static void destroy_handle(void* h) {
  try { delete (H*)h; } catch (...) {}
}
template <typename H> static const char* describe_handle(const void* h) { return h ? ((const H*)h)->describe() : ""; }
template <typename H> static int last_status_of(const void* h) { return h ? ((const H*)h)->last_status() : fc::FOURIER_HIP_INVALID_ARGUMENT; }
template <typename H> static int set_handle_option(void* h, const char* key, long long v) {
  if (!h || !key) return fc::FOURIER_HIP_INVALID_ARGUMENT;
  try { return ((H*)h)->set_option(key, v); } catch (...) { return fc::FOURIER_HIP_INVALID_ARGUMENT; }
}

#define FOURIER_DEFINE_ABI(T, SUFFIX)                                                                            \
  extern "C" fc::fourier_fft_##SUFFIX* fourier_create_##SUFFIX(size_t size) {                                    \
    return (fc::fourier_fft_##SUFFIX*)create_handle<Plan<T>>(size, -1);                                          \
  }                                                                                                              \
  extern "C" fc::fourier_fft_##SUFFIX* fourier_hip_create_##SUFFIX(size_t size, int device) {                    \
    return (fc::fourier_fft_##SUFFIX*)create_handle<Plan<T>>(size, device);                                      \
  }                                                                                                              \
  extern "C" void fourier_destroy_##SUFFIX(fc::fourier_fft_##SUFFIX* h) { destroy_handle<Plan<T>>(h); }          \
  extern "C" void fourier_transform_in_place_##SUFFIX(const fc::fourier_fft_##SUFFIX* h, std::complex<T>* x, int code) { \
    const Plan<T>* p = (const Plan<T>*)h;                                                                        \
    (void)guarded_handle(p, [&] { p->exec_host(x, x, code); });                                                  \
  }                                                                                                              \
  extern "C" void fourier_transform_##SUFFIX(const fc::fourier_fft_##SUFFIX* h, const std::complex<T>* in,       \
                                             std::complex<T>* out, int code) {                                   \
    const Plan<T>* p = (const Plan<T>*)h;                                                                        \
    (void)guarded_handle(p, [&] { p->exec_host(in, out, code); });                                               \
  }                                                                                                              \
  extern "C" size_t fourier_hip_size_##SUFFIX(const fc::fourier_fft_##SUFFIX* h) {                               \
    return h ? ((const Plan<T>*)h)->size() : 0;                                                                  \
  }                                                                                                              \
  extern "C" int fourier_hip_transform_batch_##SUFFIX(const fc::fourier_fft_##SUFFIX* h, const void* d_in,       \
                                                      void* d_out, size_t batch, int code, void* stream) {       \
    const Plan<T>* p = (const Plan<T>*)h;                                                                        \
    return guarded_handle(p, [&] { p->exec(d_in, d_out, batch, code, (hipStream_t)stream); });                   \
  }                                                                                                              \
  extern "C" int fourier_hip_reserve_##SUFFIX(const fc::fourier_fft_##SUFFIX* h, size_t batch, int in_place) {   \
    const Plan<T>* p = (const Plan<T>*)h;                                                                        \
    return guarded_handle(p, [&] { p->reserve_for(batch, in_place != 0); });                                     \
  }                                                                                                              \
  extern "C" int fourier_hip_device_##SUFFIX(const fc::fourier_fft_##SUFFIX* h) {                                \
    return h ? ((const Plan<T>*)h)->device() : -1;                                                               \
  }                                                                                                              \
  extern "C" int fourier_hip_synchronize_##SUFFIX(const fc::fourier_fft_##SUFFIX* h, void* stream) {            \
    const Plan<T>* p = (const Plan<T>*)h;                                                                        \
    return guarded_handle(p, [&] { p->synchronize((hipStream_t)stream); });                                      \
  }                                                                                                              \
  extern "C" int fourier_hip_transform_batch_host_##SUFFIX(const fc::fourier_fft_##SUFFIX* h, const std::complex<T>* in, \
                                                           std::complex<T>* out, size_t batch, int code) {      \
    const Plan<T>* p = (const Plan<T>*)h;                                                                        \
    return guarded_handle(p, [&] { p->exec_host_batch(in, out, batch, code); });                                 \
  }                                                                                                              \
  extern "C" int fourier_hip_profile_##SUFFIX(const fc::fourier_fft_##SUFFIX* h, const void* d_in, void* d_out,  \
                                              size_t batch, int code, void* stream, int nslots, float* ms_sum,   \
                                              int* launches) {                                                   \
    const Plan<T>* p = (const Plan<T>*)h;                                                                        \
    if (!ms_sum || !launches || nslots <= 0) return fc::FOURIER_HIP_INVALID_ARGUMENT;                            \
    return guarded_handle(p, [&] {                                                                               \
      Profiler prof((hipStream_t)stream);                                                                        \
      p->exec(d_in, d_out, batch, code, (hipStream_t)stream, &prof);                                             \
      prof.collect(nslots, ms_sum, launches);                                                                    \
    });                                                                                                          \
  }                                                                                                              \
  extern "C" const char* fourier_hip_slot_names_##SUFFIX(const fc::fourier_fft_##SUFFIX* h) {                    \
    static thread_local std::string s;                                                                           \
    s = h ? ((const Plan<T>*)h)->slot_names() : "";                                                              \
    return s.c_str();                                                                                            \
  }                                                                                                              \
  extern "C" int fourier_hip_last_status_##SUFFIX(const fc::fourier_fft_##SUFFIX* h) { return last_status_of<Plan<T>>(h); } \
  extern "C" int fourier_hip_set_option_##SUFFIX(fc::fourier_fft_##SUFFIX* h, const char* key, long long v) {    \
    return set_handle_option<Plan<T>>(h, key, v);                                                                \
  }                                                                                                              \
  extern "C" const char* fourier_hip_describe_##SUFFIX(const fc::fourier_fft_##SUFFIX* h) { return describe_handle<Plan<T>>(h); } \
  extern "C" double fourier_hip_model_bytes_##SUFFIX(const fc::fourier_fft_##SUFFIX* h) {                        \
    return h ? ((const Plan<T>*)h)->model_bytes() : 0.0;                                                         \
  }

FOURIER_DEFINE_ABI(float, float)
FOURIER_DEFINE_ABI(double, double)

// transforms along a strided axis (include/fourier.h, fourier_hip_transform_axis_*): methods of the complex handle, its error model
#define FOURIER_DEFINE_AXIS_ABI(T, SUFFIX)                                                                       \
  extern "C" int fourier_hip_transform_axis_##SUFFIX(const fc::fourier_fft_##SUFFIX* h, const void* d_in, void* d_out, \
                                                     size_t outer, size_t inner, int code, void* stream) {      \
    const Plan<T>* p = (const Plan<T>*)h;                                                                        \
    return guarded_handle(p, [&] { AxisRoute<T>::of(*p).transform(d_in, d_out, outer, inner, code, (hipStream_t)stream); }); \
  }                                                                                                              \
  extern "C" int fourier_hip_reserve_axis_##SUFFIX(const fc::fourier_fft_##SUFFIX* h, size_t outer, size_t inner) { \
    const Plan<T>* p = (const Plan<T>*)h;                                                                        \
    return guarded_handle(p, [&] { AxisRoute<T>::of(*p).reserve(outer, inner); });                               \
  }                                                                                                              \
  extern "C" const char* fourier_hip_describe_axis_##SUFFIX(const fc::fourier_fft_##SUFFIX* h, size_t inner) {   \
    static thread_local std::string s;                                                                           \
    s.clear();                                                                                                   \
    if (h) {                                                                                                     \
      try { s = AxisRoute<T>::of(*(const Plan<T>*)h).describe(inner); } catch (...) {}                           \
    }                                                                                                            \
    return s.c_str();                                                                                            \
  }

FOURIER_DEFINE_AXIS_ABI(float, float)
FOURIER_DEFINE_AXIS_ABI(double, double)

// The handle families built on the complex plan (include/fourier.h): the same error model.  fourier_hip_<STEM>_destroy / reserve /
// describe / last_status _<SUFFIX> on the opaque type fc::CTYPE behind which the class H stands ...
#define FOURIER_DEFINE_HANDLE_ABI(STEM, CTYPE, H, SUFFIX)                                                        \
  extern "C" void fourier_hip_##STEM##_destroy_##SUFFIX(fc::CTYPE* h) { destroy_handle<H>(h); }                  \
  extern "C" int fourier_hip_##STEM##_reserve_##SUFFIX(const fc::CTYPE* h, size_t batch) {                       \
    const H* p = (const H*)h;                                                                                    \
    return guarded_handle(p, [&] { p->reserve(batch); });                                                        \
  }                                                                                                              \
  extern "C" const char* fourier_hip_##STEM##_describe_##SUFFIX(const fc::CTYPE* h) { return describe_handle<H>(h); } \
  extern "C" int fourier_hip_##STEM##_last_status_##SUFFIX(const fc::CTYPE* h) { return last_status_of<H>(h); }
// ... and forward_batch / inverse_batch of the two real-input families
#define FOURIER_DEFINE_R2C_ABI(STEM, CTYPE, H, SUFFIX)                                                           \
  FOURIER_DEFINE_HANDLE_ABI(STEM, CTYPE, H, SUFFIX)                                                              \
  extern "C" int fourier_hip_##STEM##_forward_batch_##SUFFIX(const fc::CTYPE* h, const void* d_in, void* d_out, size_t batch, \
                                                             int code, void* stream) {                           \
    const H* p = (const H*)h;                                                                                    \
    return guarded_handle(p, [&] { p->forward(d_in, d_out, batch, code, (hipStream_t)stream); });                \
  }                                                                                                              \
  extern "C" int fourier_hip_##STEM##_inverse_batch_##SUFFIX(const fc::CTYPE* h, const void* d_in, void* d_out, size_t batch, \
                                                             int code, void* stream) {                           \
    const H* p = (const H*)h;                                                                                    \
    return guarded_handle(p, [&] { p->inverse(d_in, d_out, batch, code, (hipStream_t)stream); });                \
  }

// real-input transforms (fourier_hip_real_*)
#define FOURIER_DEFINE_REAL_ABI(T, SUFFIX)                                                                       \
  FOURIER_DEFINE_R2C_ABI(real, fourier_real_fft_##SUFFIX, RealPlan<T>, SUFFIX)                                   \
  extern "C" fc::fourier_real_fft_##SUFFIX* fourier_hip_real_create_##SUFFIX(size_t size, int device) {          \
    return (fc::fourier_real_fft_##SUFFIX*)create_handle<RealPlan<T>>(size, device);                             \
  }                                                                                                              \
  extern "C" size_t fourier_hip_real_size_##SUFFIX(const fc::fourier_real_fft_##SUFFIX* h) {                     \
    return h ? ((const RealPlan<T>*)h)->size() : 0;                                                              \
  }

FOURIER_DEFINE_REAL_ABI(float, float)
FOURIER_DEFINE_REAL_ABI(double, double)

// real-input N-D transforms (fourier_hip_realnd_*)
#define FOURIER_DEFINE_REALND_ABI(T, SUFFIX)                                                                     \
  FOURIER_DEFINE_R2C_ABI(realnd, fourier_realnd_fft_##SUFFIX, RealNdPlan<T>, SUFFIX)                             \
  extern "C" fc::fourier_realnd_fft_##SUFFIX* fourier_hip_realnd_create_##SUFFIX(int rank, const size_t* shape, int device) { \
    return (fc::fourier_realnd_fft_##SUFFIX*)create_handle<RealNdPlan<T>>(rank, shape, device);                  \
  }                                                                                                              \
  extern "C" int fourier_hip_realnd_rank_##SUFFIX(const fc::fourier_realnd_fft_##SUFFIX* h) {                    \
    return h ? ((const RealNdPlan<T>*)h)->rank() : 0;                                                            \
  }

FOURIER_DEFINE_REALND_ABI(float, float)
FOURIER_DEFINE_REALND_ABI(double, double)

// convolution with a prepared filter bank (fourier_hip_conv_*)
#define FOURIER_DEFINE_CONV_ABI(T, SUFFIX)                                                                       \
  FOURIER_DEFINE_HANDLE_ABI(conv, fourier_conv_##SUFFIX, ConvPlan<T>, SUFFIX)                                    \
  extern "C" fc::fourier_conv_##SUFFIX* fourier_hip_conv_create_##SUFFIX(size_t size, int real_data, int device) { \
    return (fc::fourier_conv_##SUFFIX*)create_handle<ConvPlan<T>>(size, real_data != 0, device);                 \
  }                                                                                                              \
  extern "C" size_t fourier_hip_conv_size_##SUFFIX(const fc::fourier_conv_##SUFFIX* h) {                         \
    return h ? ((const ConvPlan<T>*)h)->size() : 0;                                                              \
  }                                                                                                              \
  extern "C" size_t fourier_hip_conv_filters_##SUFFIX(const fc::fourier_conv_##SUFFIX* h) {                      \
    return h ? ((const ConvPlan<T>*)h)->filters() : 0;                                                           \
  }                                                                                                              \
  extern "C" int fourier_hip_conv_set_filters_##SUFFIX(fc::fourier_conv_##SUFFIX* h, const void* d_taps, size_t taps, \
                                                       size_t filters, int correlate, void* stream) {            \
    ConvPlan<T>* p = (ConvPlan<T>*)h;                                                                            \
    return guarded_handle(p, [&] { p->set_filters(d_taps, taps, filters, correlate != 0, (hipStream_t)stream); }); \
  }                                                                                                              \
  extern "C" int fourier_hip_conv_apply_##SUFFIX(const fc::fourier_conv_##SUFFIX* h, const void* d_in, void* d_out, \
                                                 size_t batch, void* stream) {                                   \
    const ConvPlan<T>* p = (const ConvPlan<T>*)h;                                                                \
    return guarded_handle(p, [&] { p->apply(d_in, d_out, batch, (hipStream_t)stream); });                        \
  }                                                                                                              \
  extern "C" int fourier_hip_conv_set_option_##SUFFIX(fc::fourier_conv_##SUFFIX* h, const char* key, long long v) { \
    return set_handle_option<ConvPlan<T>>(h, key, v);                                                            \
  }

FOURIER_DEFINE_CONV_ABI(float, float)
FOURIER_DEFINE_CONV_ABI(double, double)

// N-D convolution with a prepared filter bank (fourier_hip_convnd_*)
#define FOURIER_DEFINE_CONVND_ABI(T, SUFFIX)                                                                     \
  FOURIER_DEFINE_HANDLE_ABI(convnd, fourier_convnd_##SUFFIX, ConvNdPlan<T>, SUFFIX)                              \
  extern "C" fc::fourier_convnd_##SUFFIX* fourier_hip_convnd_create_##SUFFIX(int rank, const size_t* shape, int device) { \
    return (fc::fourier_convnd_##SUFFIX*)create_handle<ConvNdPlan<T>>(rank, shape, device);                      \
  }                                                                                                              \
  extern "C" int fourier_hip_convnd_rank_##SUFFIX(const fc::fourier_convnd_##SUFFIX* h) {                        \
    return h ? ((const ConvNdPlan<T>*)h)->rank() : 0;                                                            \
  }                                                                                                              \
  extern "C" int fourier_hip_convnd_shape_##SUFFIX(const fc::fourier_convnd_##SUFFIX* h, size_t* out) {          \
    if (!h || !out) return fc::FOURIER_HIP_INVALID_ARGUMENT;                                                     \
    const std::vector<size_t>& s = ((const ConvNdPlan<T>*)h)->shape();                                           \
    for (size_t d = 0; d < s.size(); ++d) out[d] = s[d];                                                         \
    return fc::FOURIER_HIP_OK;                                                                                   \
  }                                                                                                              \
  extern "C" size_t fourier_hip_convnd_filters_##SUFFIX(const fc::fourier_convnd_##SUFFIX* h) {                  \
    return h ? ((const ConvNdPlan<T>*)h)->filters() : 0;                                                         \
  }                                                                                                              \
  extern "C" int fourier_hip_convnd_set_filters_##SUFFIX(fc::fourier_convnd_##SUFFIX* h, const void* d_taps, const size_t* taps_shape, \
                                                         size_t filters, int correlate, void* stream) {          \
    ConvNdPlan<T>* p = (ConvNdPlan<T>*)h;                                                                        \
    return guarded_handle(p, [&] { p->set_filters(d_taps, taps_shape, filters, correlate != 0, (hipStream_t)stream); }); \
  }                                                                                                              \
  extern "C" int fourier_hip_convnd_set_window_##SUFFIX(fc::fourier_convnd_##SUFFIX* h, const size_t* in_shape,  \
                                                        const size_t* out_first, const size_t* out_shape) {      \
    ConvNdPlan<T>* p = (ConvNdPlan<T>*)h;                                                                        \
    return guarded_handle(p, [&] { p->set_window(in_shape, out_first, out_shape); });                            \
  }                                                                                                              \
  extern "C" int fourier_hip_convnd_apply_batch_##SUFFIX(const fc::fourier_convnd_##SUFFIX* h, const void* d_in, void* d_out, \
                                                         size_t batch, size_t filter_first, void* stream) {      \
    const ConvNdPlan<T>* p = (const ConvNdPlan<T>*)h;                                                            \
    return guarded_handle(p, [&] { p->apply(d_in, d_out, batch, filter_first, (hipStream_t)stream); });          \
  }                                                                                                              \
  extern "C" int fourier_hip_convnd_set_option_##SUFFIX(fc::fourier_convnd_##SUFFIX* h, const char* key, long long v) { \
    return set_handle_option<ConvNdPlan<T>>(h, key, v);                                                          \
  }

FOURIER_DEFINE_CONVND_ABI(float, float)
FOURIER_DEFINE_CONVND_ABI(double, double)

// linear convolution with a prepared filter bank (fourier_hip_lconv_*)
#define FOURIER_DEFINE_LCONV_ABI(T, SUFFIX)                                                                      \
  FOURIER_DEFINE_HANDLE_ABI(lconv, fourier_lconv_##SUFFIX, LinearConvPlan<T>, SUFFIX)                            \
  extern "C" fc::fourier_lconv_##SUFFIX* fourier_hip_lconv_create_##SUFFIX(size_t length, size_t taps, int mode, int real_data, \
                                                                           int device) {                         \
    return (fc::fourier_lconv_##SUFFIX*)create_handle<LinearConvPlan<T>>(length, taps, mode, real_data != 0, device); \
  }                                                                                                              \
  extern "C" size_t fourier_hip_lconv_length_##SUFFIX(const fc::fourier_lconv_##SUFFIX* h) {                     \
    return h ? ((const LinearConvPlan<T>*)h)->length() : 0;                                                      \
  }                                                                                                              \
  extern "C" size_t fourier_hip_lconv_taps_##SUFFIX(const fc::fourier_lconv_##SUFFIX* h) {                       \
    return h ? ((const LinearConvPlan<T>*)h)->taps() : 0;                                                        \
  }                                                                                                              \
  extern "C" size_t fourier_hip_lconv_out_length_##SUFFIX(const fc::fourier_lconv_##SUFFIX* h) {                 \
    return h ? ((const LinearConvPlan<T>*)h)->out_length() : 0;                                                  \
  }                                                                                                              \
  extern "C" size_t fourier_hip_lconv_filters_##SUFFIX(const fc::fourier_lconv_##SUFFIX* h) {                    \
    return h ? ((const LinearConvPlan<T>*)h)->filters() : 0;                                                     \
  }                                                                                                              \
  extern "C" int fourier_hip_lconv_set_filters_##SUFFIX(fc::fourier_lconv_##SUFFIX* h, const void* d_taps, size_t filters, \
                                                        int correlate, void* stream) {                           \
    LinearConvPlan<T>* p = (LinearConvPlan<T>*)h;                                                                \
    return guarded_handle(p, [&] { p->set_filters(d_taps, filters, correlate != 0, (hipStream_t)stream); });     \
  }                                                                                                              \
  extern "C" int fourier_hip_lconv_apply_##SUFFIX(const fc::fourier_lconv_##SUFFIX* h, const void* d_in, void* d_out, \
                                                  size_t batch, void* stream) {                                  \
    const LinearConvPlan<T>* p = (const LinearConvPlan<T>*)h;                                                    \
    return guarded_handle(p, [&] { p->apply(d_in, d_out, batch, (hipStream_t)stream); });                        \
  }                                                                                                              \
  extern "C" int fourier_hip_lconv_set_option_##SUFFIX(fc::fourier_lconv_##SUFFIX* h, const char* key, long long v) { \
    return set_handle_option<LinearConvPlan<T>>(h, key, v);                                                      \
  }

FOURIER_DEFINE_LCONV_ABI(float, float)
FOURIER_DEFINE_LCONV_ABI(double, double)

// real-to-real transforms, DCT / DST of types II and III (fourier_hip_r2r_*)
#define FOURIER_DEFINE_R2R_ABI(T, SUFFIX)                                                                        \
  FOURIER_DEFINE_HANDLE_ABI(r2r, fourier_r2r_##SUFFIX, R2RPlan<T>, SUFFIX)                                       \
  extern "C" fc::fourier_r2r_##SUFFIX* fourier_hip_r2r_create_##SUFFIX(size_t size, int device) {                \
    return (fc::fourier_r2r_##SUFFIX*)create_handle<R2RPlan<T>>(size, device);                                   \
  }                                                                                                              \
  extern "C" size_t fourier_hip_r2r_size_##SUFFIX(const fc::fourier_r2r_##SUFFIX* h) {                           \
    return h ? ((const R2RPlan<T>*)h)->size() : 0;                                                               \
  }                                                                                                              \
  extern "C" int fourier_hip_r2r_transform_batch_##SUFFIX(const fc::fourier_r2r_##SUFFIX* h, const void* d_in, void* d_out, \
                                                          size_t batch, int kind, int norm, void* stream) {      \
    const R2RPlan<T>* p = (const R2RPlan<T>*)h;                                                                  \
    return guarded_handle(p, [&] { p->transform(d_in, d_out, batch, kind, norm, (hipStream_t)stream); });        \
  }

FOURIER_DEFINE_R2R_ABI(float, float)
FOURIER_DEFINE_R2R_ABI(double, double)

// short-time Fourier transform and its inverse (fourier_hip_stft_*)
#define FOURIER_DEFINE_STFT_ABI(T, SUFFIX)                                                                       \
  extern "C" fc::fourier_stft_##SUFFIX* fourier_hip_stft_create_##SUFFIX(size_t n_fft, size_t hop, size_t win_length, int pad_mode, \
                                                                         int device) {                           \
    return (fc::fourier_stft_##SUFFIX*)create_handle<StftPlan<T>>(n_fft, hop, win_length, pad_mode, device);     \
  }                                                                                                              \
  extern "C" void fourier_hip_stft_destroy_##SUFFIX(fc::fourier_stft_##SUFFIX* h) { destroy_handle<StftPlan<T>>(h); } \
  extern "C" const char* fourier_hip_stft_describe_##SUFFIX(const fc::fourier_stft_##SUFFIX* h) { return describe_handle<StftPlan<T>>(h); } \
  extern "C" int fourier_hip_stft_last_status_##SUFFIX(const fc::fourier_stft_##SUFFIX* h) { return last_status_of<StftPlan<T>>(h); } \
  extern "C" int fourier_hip_stft_set_option_##SUFFIX(fc::fourier_stft_##SUFFIX* h, const char* key, long long v) { \
    return set_handle_option<StftPlan<T>>(h, key, v);                                                            \
  }                                                                                                              \
  extern "C" size_t fourier_hip_stft_n_fft_##SUFFIX(const fc::fourier_stft_##SUFFIX* h) {                        \
    return h ? ((const StftPlan<T>*)h)->n_fft() : 0;                                                             \
  }                                                                                                              \
  extern "C" size_t fourier_hip_stft_hop_##SUFFIX(const fc::fourier_stft_##SUFFIX* h) {                          \
    return h ? ((const StftPlan<T>*)h)->hop() : 0;                                                               \
  }                                                                                                              \
  extern "C" size_t fourier_hip_stft_win_length_##SUFFIX(const fc::fourier_stft_##SUFFIX* h) {                   \
    return h ? ((const StftPlan<T>*)h)->win_length() : 0;                                                        \
  }                                                                                                              \
  extern "C" size_t fourier_hip_stft_bins_##SUFFIX(const fc::fourier_stft_##SUFFIX* h) {                         \
    return h ? ((const StftPlan<T>*)h)->bins() : 0;                                                              \
  }                                                                                                              \
  extern "C" size_t fourier_hip_stft_frames_##SUFFIX(const fc::fourier_stft_##SUFFIX* h, size_t length) {        \
    return h ? ((const StftPlan<T>*)h)->frames(length) : 0;                                                      \
  }                                                                                                              \
  extern "C" int fourier_hip_stft_set_window_##SUFFIX(fc::fourier_stft_##SUFFIX* h, const void* d_window, void* stream) { \
    StftPlan<T>* p = (StftPlan<T>*)h;                                                                            \
    return guarded_handle(p, [&] { p->set_window(d_window, (hipStream_t)stream); });                             \
  }                                                                                                              \
  extern "C" int fourier_hip_stft_reserve_##SUFFIX(const fc::fourier_stft_##SUFFIX* h, size_t length, size_t batch) { \
    const StftPlan<T>* p = (const StftPlan<T>*)h;                                                                \
    return guarded_handle(p, [&] { p->reserve(length, batch); });                                                \
  }                                                                                                              \
  extern "C" int fourier_hip_stft_forward_##SUFFIX(const fc::fourier_stft_##SUFFIX* h, const void* d_in, void* d_out, size_t length, \
                                                   size_t batch, int normalized, void* stream) {                 \
    const StftPlan<T>* p = (const StftPlan<T>*)h;                                                                \
    return guarded_handle(p, [&] { p->forward(d_in, d_out, length, batch, normalized != 0, (hipStream_t)stream); }); \
  }                                                                                                              \
  extern "C" int fourier_hip_stft_inverse_##SUFFIX(const fc::fourier_stft_##SUFFIX* h, const void* d_in, void* d_out, size_t frames, \
                                                   size_t length, size_t batch, int normalized, void* stream) {  \
    const StftPlan<T>* p = (const StftPlan<T>*)h;                                                                \
    return guarded_handle(p, [&] { p->inverse(d_in, d_out, frames, length, batch, normalized != 0, (hipStream_t)stream); }); \
  }

FOURIER_DEFINE_STFT_ABI(float, float)
FOURIER_DEFINE_STFT_ABI(double, double)

// modified discrete cosine transform and its inverse (fourier_hip_mdct_*)
#define FOURIER_DEFINE_MDCT_ABI(T, SUFFIX)                                                                       \
  extern "C" fc::fourier_mdct_##SUFFIX* fourier_hip_mdct_create_##SUFFIX(size_t n, int center, int device) {     \
    return (fc::fourier_mdct_##SUFFIX*)create_handle<MdctPlan<T>>(n, center, device);                            \
  }                                                                                                              \
  extern "C" void fourier_hip_mdct_destroy_##SUFFIX(fc::fourier_mdct_##SUFFIX* h) { destroy_handle<MdctPlan<T>>(h); } \
  extern "C" const char* fourier_hip_mdct_describe_##SUFFIX(const fc::fourier_mdct_##SUFFIX* h) { return describe_handle<MdctPlan<T>>(h); } \
  extern "C" int fourier_hip_mdct_last_status_##SUFFIX(const fc::fourier_mdct_##SUFFIX* h) { return last_status_of<MdctPlan<T>>(h); } \
  extern "C" int fourier_hip_mdct_set_option_##SUFFIX(fc::fourier_mdct_##SUFFIX* h, const char* key, long long v) { \
    return set_handle_option<MdctPlan<T>>(h, key, v);                                                            \
  }                                                                                                              \
  extern "C" size_t fourier_hip_mdct_size_##SUFFIX(const fc::fourier_mdct_##SUFFIX* h) {                         \
    return h ? ((const MdctPlan<T>*)h)->size() : 0;                                                              \
  }                                                                                                              \
  extern "C" size_t fourier_hip_mdct_frames_##SUFFIX(const fc::fourier_mdct_##SUFFIX* h, size_t length) {        \
    return h ? ((const MdctPlan<T>*)h)->frames(length) : 0;                                                      \
  }                                                                                                              \
  extern "C" int fourier_hip_mdct_set_window_##SUFFIX(fc::fourier_mdct_##SUFFIX* h, const void* d_window, void* stream) { \
    MdctPlan<T>* p = (MdctPlan<T>*)h;                                                                            \
    return guarded_handle(p, [&] { p->set_window(d_window, (hipStream_t)stream); });                             \
  }                                                                                                              \
  extern "C" int fourier_hip_mdct_reserve_##SUFFIX(const fc::fourier_mdct_##SUFFIX* h, size_t length, size_t batch) { \
    const MdctPlan<T>* p = (const MdctPlan<T>*)h;                                                                \
    return guarded_handle(p, [&] { p->reserve(length, batch); });                                                \
  }                                                                                                              \
  extern "C" int fourier_hip_mdct_forward_##SUFFIX(const fc::fourier_mdct_##SUFFIX* h, const void* d_in, void* d_out, size_t length, \
                                                   size_t batch, int normalized, void* stream) {                 \
    const MdctPlan<T>* p = (const MdctPlan<T>*)h;                                                                \
    return guarded_handle(p, [&] { p->forward(d_in, d_out, length, batch, normalized != 0, (hipStream_t)stream); }); \
  }                                                                                                              \
  extern "C" int fourier_hip_mdct_inverse_##SUFFIX(const fc::fourier_mdct_##SUFFIX* h, const void* d_in, void* d_out, size_t frames, \
                                                   size_t length, size_t batch, int normalized, void* stream) {  \
    const MdctPlan<T>* p = (const MdctPlan<T>*)h;                                                                \
    return guarded_handle(p, [&] { p->inverse(d_in, d_out, frames, length, batch, normalized != 0, (hipStream_t)stream); }); \
  }

FOURIER_DEFINE_MDCT_ABI(float, float)
FOURIER_DEFINE_MDCT_ABI(double, double)

// power spectrogram and Welch average on the STFT's frames (fourier_hip_spectrogram_*)
#define FOURIER_DEFINE_SPECTROGRAM_ABI(T, SUFFIX)                                                                \
  extern "C" fc::fourier_spectrogram_##SUFFIX* fourier_hip_spectrogram_create_##SUFFIX(size_t n_fft, size_t hop, size_t win_length, int pad_mode, \
                                                                                      int device) {              \
    return (fc::fourier_spectrogram_##SUFFIX*)create_handle<SpectrogramPlan<T>>(n_fft, hop, win_length, pad_mode, device); \
  }                                                                                                              \
  extern "C" void fourier_hip_spectrogram_destroy_##SUFFIX(fc::fourier_spectrogram_##SUFFIX* h) { destroy_handle<SpectrogramPlan<T>>(h); } \
  extern "C" const char* fourier_hip_spectrogram_describe_##SUFFIX(const fc::fourier_spectrogram_##SUFFIX* h) { return describe_handle<SpectrogramPlan<T>>(h); } \
  extern "C" int fourier_hip_spectrogram_last_status_##SUFFIX(const fc::fourier_spectrogram_##SUFFIX* h) { return last_status_of<SpectrogramPlan<T>>(h); } \
  extern "C" int fourier_hip_spectrogram_set_option_##SUFFIX(fc::fourier_spectrogram_##SUFFIX* h, const char* key, long long v) { \
    return set_handle_option<SpectrogramPlan<T>>(h, key, v);                                                     \
  }                                                                                                              \
  extern "C" size_t fourier_hip_spectrogram_n_fft_##SUFFIX(const fc::fourier_spectrogram_##SUFFIX* h) {          \
    return h ? ((const SpectrogramPlan<T>*)h)->n_fft() : 0;                                                      \
  }                                                                                                              \
  extern "C" size_t fourier_hip_spectrogram_hop_##SUFFIX(const fc::fourier_spectrogram_##SUFFIX* h) {            \
    return h ? ((const SpectrogramPlan<T>*)h)->hop() : 0;                                                        \
  }                                                                                                              \
  extern "C" size_t fourier_hip_spectrogram_win_length_##SUFFIX(const fc::fourier_spectrogram_##SUFFIX* h) {     \
    return h ? ((const SpectrogramPlan<T>*)h)->win_length() : 0;                                                 \
  }                                                                                                              \
  extern "C" size_t fourier_hip_spectrogram_bins_##SUFFIX(const fc::fourier_spectrogram_##SUFFIX* h) {           \
    return h ? ((const SpectrogramPlan<T>*)h)->bins() : 0;                                                       \
  }                                                                                                              \
  extern "C" size_t fourier_hip_spectrogram_frames_##SUFFIX(const fc::fourier_spectrogram_##SUFFIX* h, size_t length) { \
    return h ? ((const SpectrogramPlan<T>*)h)->frames(length) : 0;                                               \
  }                                                                                                              \
  extern "C" int fourier_hip_spectrogram_set_window_##SUFFIX(fc::fourier_spectrogram_##SUFFIX* h, const void* d_window, void* stream) { \
    SpectrogramPlan<T>* p = (SpectrogramPlan<T>*)h;                                                              \
    return guarded_handle(p, [&] { p->set_window(d_window, (hipStream_t)stream); });                             \
  }                                                                                                              \
  extern "C" int fourier_hip_spectrogram_reserve_##SUFFIX(const fc::fourier_spectrogram_##SUFFIX* h, size_t length, size_t batch) { \
    const SpectrogramPlan<T>* p = (const SpectrogramPlan<T>*)h;                                                  \
    return guarded_handle(p, [&] { p->reserve(length, batch); });                                                \
  }                                                                                                              \
  extern "C" int fourier_hip_spectrogram_forward_##SUFFIX(const fc::fourier_spectrogram_##SUFFIX* h, const void* d_in, void* d_out, size_t length, \
                                                          size_t batch, int power, int normalized, void* stream) { \
    const SpectrogramPlan<T>* p = (const SpectrogramPlan<T>*)h;                                                  \
    return guarded_handle(p, [&] { p->forward(d_in, d_out, length, batch, power, normalized != 0, (hipStream_t)stream); }); \
  }                                                                                                              \
  extern "C" int fourier_hip_spectrogram_welch_##SUFFIX(const fc::fourier_spectrogram_##SUFFIX* h, const void* d_in, void* d_out, size_t length, \
                                                        size_t batch, int onesided_fold, double scale, void* stream) { \
    const SpectrogramPlan<T>* p = (const SpectrogramPlan<T>*)h;                                                  \
    return guarded_handle(p, [&] { p->welch(d_in, d_out, length, batch, onesided_fold != 0, scale, (hipStream_t)stream); }); \
  }

FOURIER_DEFINE_SPECTROGRAM_ABI(float, float)
FOURIER_DEFINE_SPECTROGRAM_ABI(double, double)

// cross-spectral density and coherence of two signals on the STFT's frames (fourier_hip_csd_*)
#define FOURIER_DEFINE_CSD_ABI(T, SUFFIX)                                                                        \
  extern "C" fc::fourier_csd_##SUFFIX* fourier_hip_csd_create_##SUFFIX(size_t n_fft, size_t hop, size_t win_length, int pad_mode, int device) { \
    return (fc::fourier_csd_##SUFFIX*)create_handle<CsdPlan<T>>(n_fft, hop, win_length, pad_mode, device);       \
  }                                                                                                              \
  extern "C" void fourier_hip_csd_destroy_##SUFFIX(fc::fourier_csd_##SUFFIX* h) { destroy_handle<CsdPlan<T>>(h); } \
  extern "C" const char* fourier_hip_csd_describe_##SUFFIX(const fc::fourier_csd_##SUFFIX* h) { return describe_handle<CsdPlan<T>>(h); } \
  extern "C" int fourier_hip_csd_last_status_##SUFFIX(const fc::fourier_csd_##SUFFIX* h) { return last_status_of<CsdPlan<T>>(h); } \
  extern "C" int fourier_hip_csd_set_option_##SUFFIX(fc::fourier_csd_##SUFFIX* h, const char* key, long long v) { \
    return set_handle_option<CsdPlan<T>>(h, key, v);                                                             \
  }                                                                                                              \
  extern "C" size_t fourier_hip_csd_n_fft_##SUFFIX(const fc::fourier_csd_##SUFFIX* h) { return h ? ((const CsdPlan<T>*)h)->n_fft() : 0; } \
  extern "C" size_t fourier_hip_csd_hop_##SUFFIX(const fc::fourier_csd_##SUFFIX* h) { return h ? ((const CsdPlan<T>*)h)->hop() : 0; } \
  extern "C" size_t fourier_hip_csd_win_length_##SUFFIX(const fc::fourier_csd_##SUFFIX* h) {                     \
    return h ? ((const CsdPlan<T>*)h)->win_length() : 0;                                                         \
  }                                                                                                              \
  extern "C" size_t fourier_hip_csd_bins_##SUFFIX(const fc::fourier_csd_##SUFFIX* h) { return h ? ((const CsdPlan<T>*)h)->bins() : 0; } \
  extern "C" size_t fourier_hip_csd_frames_##SUFFIX(const fc::fourier_csd_##SUFFIX* h, size_t length) {          \
    return h ? ((const CsdPlan<T>*)h)->frames(length) : 0;                                                       \
  }                                                                                                              \
  extern "C" int fourier_hip_csd_set_window_##SUFFIX(fc::fourier_csd_##SUFFIX* h, const void* d_window, void* stream) { \
    CsdPlan<T>* p = (CsdPlan<T>*)h;                                                                              \
    return guarded_handle(p, [&] { p->set_window(d_window, (hipStream_t)stream); });                             \
  }                                                                                                              \
  extern "C" int fourier_hip_csd_reserve_##SUFFIX(const fc::fourier_csd_##SUFFIX* h, size_t length, size_t batch) { \
    const CsdPlan<T>* p = (const CsdPlan<T>*)h;                                                                  \
    return guarded_handle(p, [&] { p->reserve(length, batch); });                                                \
  }                                                                                                              \
  extern "C" int fourier_hip_csd_csd_##SUFFIX(const fc::fourier_csd_##SUFFIX* h, const void* d_x, const void* d_y, void* d_out, size_t length, \
                                              size_t batch, int onesided_fold, double scale, void* stream) {     \
    const CsdPlan<T>* p = (const CsdPlan<T>*)h;                                                                  \
    return guarded_handle(p, [&] { p->csd(d_x, d_y, d_out, length, batch, onesided_fold != 0, scale, (hipStream_t)stream); }); \
  }                                                                                                              \
  extern "C" int fourier_hip_csd_coherence_##SUFFIX(const fc::fourier_csd_##SUFFIX* h, const void* d_x, const void* d_y, void* d_out, \
                                                    size_t length, size_t batch, void* stream) {                 \
    const CsdPlan<T>* p = (const CsdPlan<T>*)h;                                                                  \
    return guarded_handle(p, [&] { p->coherence(d_x, d_y, d_out, length, batch, (hipStream_t)stream); });        \
  }

FOURIER_DEFINE_CSD_ABI(float, float)
FOURIER_DEFINE_CSD_ABI(double, double)

// band-energy (mel) spectrogram on the STFT's frames (fourier_hip_bandspec_*)
#define FOURIER_DEFINE_BANDSPEC_ABI(T, SUFFIX)                                                                   \
  extern "C" fc::fourier_bandspec_##SUFFIX* fourier_hip_bandspec_create_##SUFFIX(size_t n_fft, size_t hop, size_t win_length, int pad_mode, \
                                                                                size_t bands, int device) {      \
    return (fc::fourier_bandspec_##SUFFIX*)create_handle<BandSpecPlan<T>>(n_fft, hop, win_length, pad_mode, bands, device); \
  }                                                                                                              \
  extern "C" void fourier_hip_bandspec_destroy_##SUFFIX(fc::fourier_bandspec_##SUFFIX* h) { destroy_handle<BandSpecPlan<T>>(h); } \
  extern "C" const char* fourier_hip_bandspec_describe_##SUFFIX(const fc::fourier_bandspec_##SUFFIX* h) { return describe_handle<BandSpecPlan<T>>(h); } \
  extern "C" int fourier_hip_bandspec_last_status_##SUFFIX(const fc::fourier_bandspec_##SUFFIX* h) { return last_status_of<BandSpecPlan<T>>(h); } \
  extern "C" int fourier_hip_bandspec_set_option_##SUFFIX(fc::fourier_bandspec_##SUFFIX* h, const char* key, long long v) { \
    return set_handle_option<BandSpecPlan<T>>(h, key, v);                                                        \
  }                                                                                                              \
  extern "C" size_t fourier_hip_bandspec_n_fft_##SUFFIX(const fc::fourier_bandspec_##SUFFIX* h) { return h ? ((const BandSpecPlan<T>*)h)->n_fft() : 0; } \
  extern "C" size_t fourier_hip_bandspec_hop_##SUFFIX(const fc::fourier_bandspec_##SUFFIX* h) { return h ? ((const BandSpecPlan<T>*)h)->hop() : 0; } \
  extern "C" size_t fourier_hip_bandspec_win_length_##SUFFIX(const fc::fourier_bandspec_##SUFFIX* h) {           \
    return h ? ((const BandSpecPlan<T>*)h)->win_length() : 0;                                                    \
  }                                                                                                              \
  extern "C" size_t fourier_hip_bandspec_bins_##SUFFIX(const fc::fourier_bandspec_##SUFFIX* h) { return h ? ((const BandSpecPlan<T>*)h)->bins() : 0; } \
  extern "C" size_t fourier_hip_bandspec_bands_##SUFFIX(const fc::fourier_bandspec_##SUFFIX* h) { return h ? ((const BandSpecPlan<T>*)h)->bands() : 0; } \
  extern "C" size_t fourier_hip_bandspec_frames_##SUFFIX(const fc::fourier_bandspec_##SUFFIX* h, size_t length) { \
    return h ? ((const BandSpecPlan<T>*)h)->frames(length) : 0;                                                  \
  }                                                                                                              \
  extern "C" int fourier_hip_bandspec_set_window_##SUFFIX(fc::fourier_bandspec_##SUFFIX* h, const void* d_window, void* stream) { \
    BandSpecPlan<T>* p = (BandSpecPlan<T>*)h;                                                                    \
    return guarded_handle(p, [&] { p->set_window(d_window, (hipStream_t)stream); });                             \
  }                                                                                                              \
  extern "C" int fourier_hip_bandspec_set_bands_##SUFFIX(fc::fourier_bandspec_##SUFFIX* h, const void* h_matrix, void* stream) { \
    BandSpecPlan<T>* p = (BandSpecPlan<T>*)h;                                                                    \
    return guarded_handle(p, [&] { p->set_bands(h_matrix, (hipStream_t)stream); });                              \
  }                                                                                                              \
  extern "C" int fourier_hip_bandspec_reserve_##SUFFIX(const fc::fourier_bandspec_##SUFFIX* h, size_t length, size_t batch) { \
    const BandSpecPlan<T>* p = (const BandSpecPlan<T>*)h;                                                        \
    return guarded_handle(p, [&] { p->reserve(length, batch); });                                                \
  }                                                                                                              \
  extern "C" int fourier_hip_bandspec_forward_##SUFFIX(const fc::fourier_bandspec_##SUFFIX* h, const void* d_in, void* d_out, size_t length, \
                                                       size_t batch, int power, int normalized, double log_mult, double log_floor, \
                                                       void* stream) {                                           \
    const BandSpecPlan<T>* p = (const BandSpecPlan<T>*)h;                                                        \
    return guarded_handle(p, [&] { p->forward(d_in, d_out, length, batch, power, normalized != 0, log_mult, log_floor, (hipStream_t)stream); }); \
  }

FOURIER_DEFINE_BANDSPEC_ABI(float, float)
FOURIER_DEFINE_BANDSPEC_ABI(double, double)

// analytic signal and envelope of real rows (fourier_hip_hilbert_*)
#define FOURIER_DEFINE_HILBERT_ABI(T, SUFFIX)                                                                    \
  FOURIER_DEFINE_HANDLE_ABI(hilbert, fourier_hilbert_##SUFFIX, HilbertPlan<T>, SUFFIX)                           \
  extern "C" fc::fourier_hilbert_##SUFFIX* fourier_hip_hilbert_create_##SUFFIX(size_t size, int device) {        \
    return (fc::fourier_hilbert_##SUFFIX*)create_handle<HilbertPlan<T>>(size, device);                           \
  }                                                                                                              \
  extern "C" size_t fourier_hip_hilbert_size_##SUFFIX(const fc::fourier_hilbert_##SUFFIX* h) {                   \
    return h ? ((const HilbertPlan<T>*)h)->size() : 0;                                                           \
  }                                                                                                              \
  extern "C" int fourier_hip_hilbert_analytic_##SUFFIX(const fc::fourier_hilbert_##SUFFIX* h, const void* d_in, void* d_out, \
                                                       size_t batch, void* stream) {                             \
    const HilbertPlan<T>* p = (const HilbertPlan<T>*)h;                                                          \
    return guarded_handle(p, [&] { p->analytic(d_in, d_out, batch, (hipStream_t)stream); });                     \
  }                                                                                                              \
  extern "C" int fourier_hip_hilbert_envelope_##SUFFIX(const fc::fourier_hilbert_##SUFFIX* h, const void* d_in, void* d_out, \
                                                       size_t batch, void* stream) {                             \
    const HilbertPlan<T>* p = (const HilbertPlan<T>*)h;                                                          \
    return guarded_handle(p, [&] { p->envelope(d_in, d_out, batch, (hipStream_t)stream); });                     \
  }                                                                                                              \
  extern "C" int fourier_hip_hilbert_set_option_##SUFFIX(fc::fourier_hilbert_##SUFFIX* h, const char* key, long long v) { \
    return set_handle_option<HilbertPlan<T>>(h, key, v);                                                         \
  }

FOURIER_DEFINE_HILBERT_ABI(float, float)
FOURIER_DEFINE_HILBERT_ABI(double, double)

// chirp-z transform and zoom FFT (fourier_hip_czt_*)
#define FOURIER_DEFINE_CZT_ABI(T, SUFFIX)                                                                        \
  FOURIER_DEFINE_HANDLE_ABI(czt, fourier_czt_##SUFFIX, CztPlan<T>, SUFFIX)                                       \
  extern "C" fc::fourier_czt_##SUFFIX* fourier_hip_czt_create_##SUFFIX(size_t n, size_t m, double w_abs, double w_turns, double a_abs, \
                                                                       double a_turns, int real_input, int device) { \
    return (fc::fourier_czt_##SUFFIX*)create_handle<CztPlan<T>>(n, m, w_abs, w_turns, a_abs, a_turns, real_input != 0, device); \
  }                                                                                                              \
  extern "C" size_t fourier_hip_czt_size_##SUFFIX(const fc::fourier_czt_##SUFFIX* h) {                           \
    return h ? ((const CztPlan<T>*)h)->size() : 0;                                                               \
  }                                                                                                              \
  extern "C" size_t fourier_hip_czt_points_##SUFFIX(const fc::fourier_czt_##SUFFIX* h) {                         \
    return h ? ((const CztPlan<T>*)h)->points() : 0;                                                             \
  }                                                                                                              \
  extern "C" int fourier_hip_czt_transform_##SUFFIX(const fc::fourier_czt_##SUFFIX* h, const void* d_in, void* d_out, size_t batch, \
                                                    void* stream) {                                              \
    const CztPlan<T>* p = (const CztPlan<T>*)h;                                                                  \
    return guarded_handle(p, [&] { p->transform(d_in, d_out, batch, (hipStream_t)stream); });                    \
  }                                                                                                              \
  extern "C" int fourier_hip_czt_set_option_##SUFFIX(fc::fourier_czt_##SUFFIX* h, const char* key, long long v) { \
    return set_handle_option<CztPlan<T>>(h, key, v);                                                             \
  }

FOURIER_DEFINE_CZT_ABI(float, float)
FOURIER_DEFINE_CZT_ABI(double, double)

// polyphase filter bank channelizer (fourier_hip_pfb_*)
#define FOURIER_DEFINE_PFB_ABI(T, SUFFIX)                                                                        \
  extern "C" fc::fourier_pfb_##SUFFIX* fourier_hip_pfb_create_##SUFFIX(size_t channels, size_t taps, size_t hop, int real_input, int device) { \
    return (fc::fourier_pfb_##SUFFIX*)create_handle<PfbPlan<T>>(channels, taps, hop, real_input, device);        \
  }                                                                                                              \
  extern "C" void fourier_hip_pfb_destroy_##SUFFIX(fc::fourier_pfb_##SUFFIX* h) { destroy_handle<PfbPlan<T>>(h); } \
  extern "C" const char* fourier_hip_pfb_describe_##SUFFIX(const fc::fourier_pfb_##SUFFIX* h) { return describe_handle<PfbPlan<T>>(h); } \
  extern "C" int fourier_hip_pfb_last_status_##SUFFIX(const fc::fourier_pfb_##SUFFIX* h) { return last_status_of<PfbPlan<T>>(h); } \
  extern "C" int fourier_hip_pfb_set_option_##SUFFIX(fc::fourier_pfb_##SUFFIX* h, const char* key, long long v) { \
    return set_handle_option<PfbPlan<T>>(h, key, v);                                                             \
  }                                                                                                              \
  extern "C" size_t fourier_hip_pfb_channels_##SUFFIX(const fc::fourier_pfb_##SUFFIX* h) {                       \
    return h ? ((const PfbPlan<T>*)h)->channels() : 0;                                                           \
  }                                                                                                              \
  extern "C" size_t fourier_hip_pfb_taps_##SUFFIX(const fc::fourier_pfb_##SUFFIX* h) {                           \
    return h ? ((const PfbPlan<T>*)h)->taps() : 0;                                                               \
  }                                                                                                              \
  extern "C" size_t fourier_hip_pfb_hop_##SUFFIX(const fc::fourier_pfb_##SUFFIX* h) {                            \
    return h ? ((const PfbPlan<T>*)h)->hop() : 0;                                                                \
  }                                                                                                              \
  extern "C" size_t fourier_hip_pfb_bins_##SUFFIX(const fc::fourier_pfb_##SUFFIX* h) {                           \
    return h ? ((const PfbPlan<T>*)h)->bins() : 0;                                                               \
  }                                                                                                              \
  extern "C" size_t fourier_hip_pfb_frames_##SUFFIX(const fc::fourier_pfb_##SUFFIX* h, size_t length) {          \
    return h ? ((const PfbPlan<T>*)h)->frames(length) : 0;                                                       \
  }                                                                                                              \
  extern "C" int fourier_hip_pfb_set_filter_##SUFFIX(fc::fourier_pfb_##SUFFIX* h, const void* d_filter, void* stream) { \
    PfbPlan<T>* p = (PfbPlan<T>*)h;                                                                              \
    return guarded_handle(p, [&] { p->set_filter(d_filter, (hipStream_t)stream); });                             \
  }                                                                                                              \
  extern "C" int fourier_hip_pfb_reserve_##SUFFIX(const fc::fourier_pfb_##SUFFIX* h, size_t length, size_t batch) { \
    const PfbPlan<T>* p = (const PfbPlan<T>*)h;                                                                  \
    return guarded_handle(p, [&] { p->reserve(length, batch); });                                                \
  }                                                                                                              \
  extern "C" int fourier_hip_pfb_forward_##SUFFIX(const fc::fourier_pfb_##SUFFIX* h, const void* d_in, void* d_out, size_t length, \
                                                  size_t batch, void* stream) {                                  \
    const PfbPlan<T>* p = (const PfbPlan<T>*)h;                                                                  \
    return guarded_handle(p, [&] { p->forward(d_in, d_out, length, batch, (hipStream_t)stream); });              \
  }

FOURIER_DEFINE_PFB_ABI(float, float)
FOURIER_DEFINE_PFB_ABI(double, double)

// polyphase synthesis filter bank (fourier_hip_ipfb_*)
#define FOURIER_DEFINE_IPFB_ABI(T, SUFFIX)                                                                       \
  extern "C" fc::fourier_ipfb_##SUFFIX* fourier_hip_ipfb_create_##SUFFIX(size_t channels, size_t taps, size_t hop, int real_output, int device) { \
    return (fc::fourier_ipfb_##SUFFIX*)create_handle<IpfbPlan<T>>(channels, taps, hop, real_output, device);     \
  }                                                                                                              \
  extern "C" void fourier_hip_ipfb_destroy_##SUFFIX(fc::fourier_ipfb_##SUFFIX* h) { destroy_handle<IpfbPlan<T>>(h); } \
  extern "C" const char* fourier_hip_ipfb_describe_##SUFFIX(const fc::fourier_ipfb_##SUFFIX* h) { return describe_handle<IpfbPlan<T>>(h); } \
  extern "C" int fourier_hip_ipfb_last_status_##SUFFIX(const fc::fourier_ipfb_##SUFFIX* h) { return last_status_of<IpfbPlan<T>>(h); } \
  extern "C" size_t fourier_hip_ipfb_channels_##SUFFIX(const fc::fourier_ipfb_##SUFFIX* h) {                     \
    return h ? ((const IpfbPlan<T>*)h)->channels() : 0;                                                          \
  }                                                                                                              \
  extern "C" size_t fourier_hip_ipfb_taps_##SUFFIX(const fc::fourier_ipfb_##SUFFIX* h) {                         \
    return h ? ((const IpfbPlan<T>*)h)->taps() : 0;                                                              \
  }                                                                                                              \
  extern "C" size_t fourier_hip_ipfb_hop_##SUFFIX(const fc::fourier_ipfb_##SUFFIX* h) {                          \
    return h ? ((const IpfbPlan<T>*)h)->hop() : 0;                                                               \
  }                                                                                                              \
  extern "C" size_t fourier_hip_ipfb_bins_##SUFFIX(const fc::fourier_ipfb_##SUFFIX* h) {                         \
    return h ? ((const IpfbPlan<T>*)h)->bins() : 0;                                                              \
  }                                                                                                              \
  extern "C" size_t fourier_hip_ipfb_length_##SUFFIX(const fc::fourier_ipfb_##SUFFIX* h, size_t frames) {        \
    return h ? ((const IpfbPlan<T>*)h)->length(frames) : 0;                                                      \
  }                                                                                                              \
  extern "C" int fourier_hip_ipfb_set_filter_##SUFFIX(fc::fourier_ipfb_##SUFFIX* h, const void* d_filter, void* stream) { \
    IpfbPlan<T>* p = (IpfbPlan<T>*)h;                                                                            \
    return guarded_handle(p, [&] { p->set_filter(d_filter, (hipStream_t)stream); });                             \
  }                                                                                                              \
  extern "C" int fourier_hip_ipfb_reserve_##SUFFIX(const fc::fourier_ipfb_##SUFFIX* h, size_t frames, size_t batch) { \
    const IpfbPlan<T>* p = (const IpfbPlan<T>*)h;                                                                \
    return guarded_handle(p, [&] { p->reserve(frames, batch); });                                                \
  }                                                                                                              \
  extern "C" int fourier_hip_ipfb_inverse_##SUFFIX(const fc::fourier_ipfb_##SUFFIX* h, const void* d_in, void* d_out, size_t frames, \
                                                   size_t length, size_t batch, void* stream) {                  \
    const IpfbPlan<T>* p = (const IpfbPlan<T>*)h;                                                                \
    return guarded_handle(p, [&] { p->inverse(d_in, d_out, frames, length, batch, (hipStream_t)stream); });      \
  }

FOURIER_DEFINE_IPFB_ABI(float, float)
FOURIER_DEFINE_IPFB_ABI(double, double)

// Fourier-domain resampling of complex or real rows (fourier_hip_resample_*)
#define FOURIER_DEFINE_RESAMPLE_ABI(T, SUFFIX)                                                                   \
  FOURIER_DEFINE_HANDLE_ABI(resample, fourier_resample_##SUFFIX, ResamplePlan<T>, SUFFIX)                        \
  extern "C" fc::fourier_resample_##SUFFIX* fourier_hip_resample_create_##SUFFIX(size_t n_in, size_t n_out, int real_input, int device) { \
    return (fc::fourier_resample_##SUFFIX*)create_handle<ResamplePlan<T>>(n_in, n_out, real_input, device);      \
  }                                                                                                              \
  extern "C" size_t fourier_hip_resample_size_in_##SUFFIX(const fc::fourier_resample_##SUFFIX* h) {              \
    return h ? ((const ResamplePlan<T>*)h)->size_in() : 0;                                                       \
  }                                                                                                              \
  extern "C" size_t fourier_hip_resample_size_out_##SUFFIX(const fc::fourier_resample_##SUFFIX* h) {             \
    return h ? ((const ResamplePlan<T>*)h)->size_out() : 0;                                                      \
  }                                                                                                              \
  extern "C" int fourier_hip_resample_real_input_##SUFFIX(const fc::fourier_resample_##SUFFIX* h) {              \
    return h ? (int)((const ResamplePlan<T>*)h)->real_input() : 0;                                               \
  }                                                                                                              \
  extern "C" int fourier_hip_resample_forward_##SUFFIX(const fc::fourier_resample_##SUFFIX* h, const void* d_in, void* d_out, \
                                                       size_t batch, void* stream) {                             \
    const ResamplePlan<T>* p = (const ResamplePlan<T>*)h;                                                        \
    return guarded_handle(p, [&] { p->forward(d_in, d_out, batch, (hipStream_t)stream); });                      \
  }                                                                                                              \
  extern "C" int fourier_hip_resample_set_window_##SUFFIX(fc::fourier_resample_##SUFFIX* h, const void* d_window, void* stream) { \
    ResamplePlan<T>* p = (ResamplePlan<T>*)h;                                                                    \
    return guarded_handle(p, [&] { p->set_window(d_window, (hipStream_t)stream); });                             \
  }                                                                                                              \
  extern "C" int fourier_hip_resample_set_option_##SUFFIX(fc::fourier_resample_##SUFFIX* h, const char* key, long long v) { \
    return set_handle_option<ResamplePlan<T>>(h, key, v);                                                        \
  }

FOURIER_DEFINE_RESAMPLE_ABI(float, float)
FOURIER_DEFINE_RESAMPLE_ABI(double, double)

// pairwise cross-correlation and GCC-PHAT (fourier_hip_xcorr_*)
#define FOURIER_DEFINE_XCORR_ABI(T, SUFFIX)                                                                      \
  FOURIER_DEFINE_HANDLE_ABI(xcorr, fourier_xcorr_##SUFFIX, XcorrPlan<T>, SUFFIX)                                 \
  extern "C" fc::fourier_xcorr_##SUFFIX* fourier_hip_xcorr_create_##SUFFIX(size_t size, size_t length, long long lag_first, size_t lags, \
                                                                           int real_data, int device) {         \
    return (fc::fourier_xcorr_##SUFFIX*)create_handle<XcorrPlan<T>>(size, length, lag_first, lags, real_data, device); \
  }                                                                                                              \
  extern "C" size_t fourier_hip_xcorr_size_##SUFFIX(const fc::fourier_xcorr_##SUFFIX* h) {                       \
    return h ? ((const XcorrPlan<T>*)h)->size() : 0;                                                             \
  }                                                                                                              \
  extern "C" size_t fourier_hip_xcorr_length_##SUFFIX(const fc::fourier_xcorr_##SUFFIX* h) {                     \
    return h ? ((const XcorrPlan<T>*)h)->length() : 0;                                                           \
  }                                                                                                              \
  extern "C" size_t fourier_hip_xcorr_lags_##SUFFIX(const fc::fourier_xcorr_##SUFFIX* h) {                       \
    return h ? ((const XcorrPlan<T>*)h)->lags() : 0;                                                             \
  }                                                                                                              \
  extern "C" int fourier_hip_xcorr_correlate_##SUFFIX(const fc::fourier_xcorr_##SUFFIX* h, const void* d_x, const void* d_y, void* d_out, \
                                                      size_t batch, void* stream) {                              \
    const XcorrPlan<T>* p = (const XcorrPlan<T>*)h;                                                              \
    return guarded_handle(p, [&] { p->correlate(d_x, d_y, d_out, batch, (hipStream_t)stream); });                \
  }                                                                                                              \
  extern "C" int fourier_hip_xcorr_set_option_##SUFFIX(fc::fourier_xcorr_##SUFFIX* h, const char* key, long long v) { \
    return set_handle_option<XcorrPlan<T>>(h, key, v);                                                           \
  }

FOURIER_DEFINE_XCORR_ABI(float, float)
FOURIER_DEFINE_XCORR_ABI(double, double)

// fractional delay and delay-and-sum (fourier_hip_delay_*)
#define FOURIER_DEFINE_DELAY_ABI(T, SUFFIX)                                                                      \
  FOURIER_DEFINE_HANDLE_ABI(delay, fourier_delay_##SUFFIX, DelayPlan<T>, SUFFIX)                                 \
  extern "C" fc::fourier_delay_##SUFFIX* fourier_hip_delay_create_##SUFFIX(size_t size, size_t length, size_t channels, int real_data, \
                                                                           int device) {                        \
    return (fc::fourier_delay_##SUFFIX*)create_handle<DelayPlan<T>>(size, length, channels, real_data, device);  \
  }                                                                                                              \
  extern "C" size_t fourier_hip_delay_size_##SUFFIX(const fc::fourier_delay_##SUFFIX* h) {                       \
    return h ? ((const DelayPlan<T>*)h)->size() : 0;                                                             \
  }                                                                                                              \
  extern "C" size_t fourier_hip_delay_length_##SUFFIX(const fc::fourier_delay_##SUFFIX* h) {                     \
    return h ? ((const DelayPlan<T>*)h)->length() : 0;                                                           \
  }                                                                                                              \
  extern "C" size_t fourier_hip_delay_channels_##SUFFIX(const fc::fourier_delay_##SUFFIX* h) {                   \
    return h ? ((const DelayPlan<T>*)h)->channels() : 0;                                                         \
  }                                                                                                              \
  extern "C" int fourier_hip_delay_apply_##SUFFIX(const fc::fourier_delay_##SUFFIX* h, const void* d_in, const void* d_delays, \
                                                  const void* d_weights, void* d_out, size_t batch, void* stream) { \
    const DelayPlan<T>* p = (const DelayPlan<T>*)h;                                                              \
    return guarded_handle(p, [&] { p->apply(d_in, d_delays, d_weights, d_out, batch, (hipStream_t)stream); });   \
  }                                                                                                              \
  extern "C" int fourier_hip_delay_set_option_##SUFFIX(fc::fourier_delay_##SUFFIX* h, const char* key, long long v) { \
    return set_handle_option<DelayPlan<T>>(h, key, v);                                                           \
  }

FOURIER_DEFINE_DELAY_ABI(float, float)
FOURIER_DEFINE_DELAY_ABI(double, double)

// real cepstrum and minimum-phase reconstruction (fourier_hip_cepstrum_*)
#define FOURIER_DEFINE_CEPSTRUM_ABI(T, SUFFIX)                                                                   \
  FOURIER_DEFINE_HANDLE_ABI(cepstrum, fourier_cepstrum_##SUFFIX, CepstrumPlan<T>, SUFFIX)                        \
  extern "C" fc::fourier_cepstrum_##SUFFIX* fourier_hip_cepstrum_create_##SUFFIX(size_t size, size_t length, size_t outputs, int mode, \
                                                                                 int device) {                  \
    return (fc::fourier_cepstrum_##SUFFIX*)create_handle<CepstrumPlan<T>>(size, length, outputs, mode, device);  \
  }                                                                                                              \
  extern "C" size_t fourier_hip_cepstrum_size_##SUFFIX(const fc::fourier_cepstrum_##SUFFIX* h) {                 \
    return h ? ((const CepstrumPlan<T>*)h)->size() : 0;                                                          \
  }                                                                                                              \
  extern "C" size_t fourier_hip_cepstrum_length_##SUFFIX(const fc::fourier_cepstrum_##SUFFIX* h) {               \
    return h ? ((const CepstrumPlan<T>*)h)->length() : 0;                                                        \
  }                                                                                                              \
  extern "C" size_t fourier_hip_cepstrum_outputs_##SUFFIX(const fc::fourier_cepstrum_##SUFFIX* h) {              \
    return h ? ((const CepstrumPlan<T>*)h)->outputs() : 0;                                                       \
  }                                                                                                              \
  extern "C" int fourier_hip_cepstrum_mode_##SUFFIX(const fc::fourier_cepstrum_##SUFFIX* h) {                    \
    return h ? ((const CepstrumPlan<T>*)h)->mode() : -1;                                                         \
  }                                                                                                              \
  extern "C" int fourier_hip_cepstrum_apply_##SUFFIX(const fc::fourier_cepstrum_##SUFFIX* h, const void* d_in, void* d_out, \
                                                     size_t batch, double log_mult, double log_floor, void* stream) { \
    const CepstrumPlan<T>* p = (const CepstrumPlan<T>*)h;                                                        \
    return guarded_handle(p, [&] { p->apply(d_in, d_out, batch, log_mult, log_floor, (hipStream_t)stream); });   \
  }                                                                                                              \
  extern "C" int fourier_hip_cepstrum_set_option_##SUFFIX(fc::fourier_cepstrum_##SUFFIX* h, const char* key, long long v) { \
    return set_handle_option<CepstrumPlan<T>>(h, key, v);                                                        \
  }

FOURIER_DEFINE_CEPSTRUM_ABI(float, float)
FOURIER_DEFINE_CEPSTRUM_ABI(double, double)

// non-uniform FFT, 1-D types 1 and 2 (fourier_hip_nufft_*)
#define FOURIER_DEFINE_NUFFT_ABI(T, SUFFIX)                                                                      \
  FOURIER_DEFINE_HANDLE_ABI(nufft, fourier_nufft_##SUFFIX, NufftPlan<T>, SUFFIX)                                 \
  extern "C" fc::fourier_nufft_##SUFFIX* fourier_hip_nufft_create_##SUFFIX(size_t n_modes, double eps, int device) { \
    return (fc::fourier_nufft_##SUFFIX*)create_handle<NufftPlan<T>>(n_modes, eps, device);                       \
  }                                                                                                              \
  extern "C" size_t fourier_hip_nufft_modes_##SUFFIX(const fc::fourier_nufft_##SUFFIX* h) {                      \
    return h ? ((const NufftPlan<T>*)h)->modes() : 0;                                                            \
  }                                                                                                              \
  extern "C" size_t fourier_hip_nufft_points_##SUFFIX(const fc::fourier_nufft_##SUFFIX* h) {                     \
    return h ? ((const NufftPlan<T>*)h)->points() : 0;                                                           \
  }                                                                                                              \
  extern "C" int fourier_hip_nufft_set_points_##SUFFIX(fc::fourier_nufft_##SUFFIX* h, const double* h_points, size_t m, void* stream) { \
    NufftPlan<T>* p = (NufftPlan<T>*)h;                                                                          \
    return guarded_handle(p, [&] { p->set_points(h_points, m, (hipStream_t)stream); });                          \
  }                                                                                                              \
  extern "C" int fourier_hip_nufft_to_modes_batch_##SUFFIX(const fc::fourier_nufft_##SUFFIX* h, const void* d_in, void* d_out, \
                                                           size_t batch, int sign, int order, void* stream) {    \
    const NufftPlan<T>* p = (const NufftPlan<T>*)h;                                                              \
    return guarded_handle(p, [&] { p->to_modes(d_in, d_out, batch, sign, order, (hipStream_t)stream); });        \
  }                                                                                                              \
  extern "C" int fourier_hip_nufft_to_points_batch_##SUFFIX(const fc::fourier_nufft_##SUFFIX* h, const void* d_in, void* d_out, \
                                                            size_t batch, int sign, int order, void* stream) {   \
    const NufftPlan<T>* p = (const NufftPlan<T>*)h;                                                              \
    return guarded_handle(p, [&] { p->to_points(d_in, d_out, batch, sign, order, (hipStream_t)stream); });       \
  }                                                                                                              \
  extern "C" int fourier_hip_nufft_set_option_##SUFFIX(fc::fourier_nufft_##SUFFIX* h, const char* key, long long v) { \
    return set_handle_option<NufftPlan<T>>(h, key, v);                                                           \
  }

FOURIER_DEFINE_NUFFT_ABI(float, float)
FOURIER_DEFINE_NUFFT_ABI(double, double)

// non-uniform FFT, 2-D types 1 and 2 (fourier_hip_nufft2d_*)
#define FOURIER_DEFINE_NUFFT2D_ABI(T, SUFFIX)                                                                    \
  FOURIER_DEFINE_HANDLE_ABI(nufft2d, fourier_nufft2d_##SUFFIX, Nufft2dPlan<T>, SUFFIX)                           \
  extern "C" fc::fourier_nufft2d_##SUFFIX* fourier_hip_nufft2d_create_##SUFFIX(size_t n1, size_t n2, double eps, int device) { \
    return (fc::fourier_nufft2d_##SUFFIX*)create_handle<Nufft2dPlan<T>>(n1, n2, eps, device);                    \
  }                                                                                                              \
  extern "C" size_t fourier_hip_nufft2d_modes1_##SUFFIX(const fc::fourier_nufft2d_##SUFFIX* h) {                 \
    return h ? ((const Nufft2dPlan<T>*)h)->modes1() : 0;                                                         \
  }                                                                                                              \
  extern "C" size_t fourier_hip_nufft2d_modes2_##SUFFIX(const fc::fourier_nufft2d_##SUFFIX* h) {                 \
    return h ? ((const Nufft2dPlan<T>*)h)->modes2() : 0;                                                         \
  }                                                                                                              \
  extern "C" size_t fourier_hip_nufft2d_points_##SUFFIX(const fc::fourier_nufft2d_##SUFFIX* h) {                 \
    return h ? ((const Nufft2dPlan<T>*)h)->points() : 0;                                                         \
  }                                                                                                              \
  extern "C" int fourier_hip_nufft2d_set_points_##SUFFIX(fc::fourier_nufft2d_##SUFFIX* h, const double* h_x1, const double* h_x2, \
                                                         size_t m, void* stream) {                               \
    Nufft2dPlan<T>* p = (Nufft2dPlan<T>*)h;                                                                      \
    return guarded_handle(p, [&] { p->set_points(h_x1, h_x2, m, (hipStream_t)stream); });                        \
  }                                                                                                              \
  extern "C" int fourier_hip_nufft2d_to_modes_batch_##SUFFIX(const fc::fourier_nufft2d_##SUFFIX* h, const void* d_in, void* d_out, \
                                                             size_t batch, int sign, int order, void* stream) {  \
    const Nufft2dPlan<T>* p = (const Nufft2dPlan<T>*)h;                                                          \
    return guarded_handle(p, [&] { p->to_modes(d_in, d_out, batch, sign, order, (hipStream_t)stream); });        \
  }                                                                                                              \
  extern "C" int fourier_hip_nufft2d_to_points_batch_##SUFFIX(const fc::fourier_nufft2d_##SUFFIX* h, const void* d_in, void* d_out, \
                                                              size_t batch, int sign, int order, void* stream) { \
    const Nufft2dPlan<T>* p = (const Nufft2dPlan<T>*)h;                                                          \
    return guarded_handle(p, [&] { p->to_points(d_in, d_out, batch, sign, order, (hipStream_t)stream); });       \
  }                                                                                                              \
  extern "C" int fourier_hip_nufft2d_set_option_##SUFFIX(fc::fourier_nufft2d_##SUFFIX* h, const char* key, long long v) { \
    return set_handle_option<Nufft2dPlan<T>>(h, key, v);                                                         \
  }

FOURIER_DEFINE_NUFFT2D_ABI(float, float)
FOURIER_DEFINE_NUFFT2D_ABI(double, double)

// non-uniform FFT, 3-D types 1 and 2 (fourier_hip_nufft3d_*)
#define FOURIER_DEFINE_NUFFT3D_ABI(T, SUFFIX)                                                                    \
  FOURIER_DEFINE_HANDLE_ABI(nufft3d, fourier_nufft3d_##SUFFIX, Nufft3dPlan<T>, SUFFIX)                           \
  extern "C" fc::fourier_nufft3d_##SUFFIX* fourier_hip_nufft3d_create_##SUFFIX(size_t n1, size_t n2, size_t n3, double eps, int device) { \
    return (fc::fourier_nufft3d_##SUFFIX*)create_handle<Nufft3dPlan<T>>(n1, n2, n3, eps, device);                \
  }                                                                                                              \
  extern "C" size_t fourier_hip_nufft3d_modes1_##SUFFIX(const fc::fourier_nufft3d_##SUFFIX* h) {                 \
    return h ? ((const Nufft3dPlan<T>*)h)->modes1() : 0;                                                         \
  }                                                                                                              \
  extern "C" size_t fourier_hip_nufft3d_modes2_##SUFFIX(const fc::fourier_nufft3d_##SUFFIX* h) {                 \
    return h ? ((const Nufft3dPlan<T>*)h)->modes2() : 0;                                                         \
  }                                                                                                              \
  extern "C" size_t fourier_hip_nufft3d_modes3_##SUFFIX(const fc::fourier_nufft3d_##SUFFIX* h) {                 \
    return h ? ((const Nufft3dPlan<T>*)h)->modes3() : 0;                                                         \
  }                                                                                                              \
  extern "C" size_t fourier_hip_nufft3d_points_##SUFFIX(const fc::fourier_nufft3d_##SUFFIX* h) {                 \
    return h ? ((const Nufft3dPlan<T>*)h)->points() : 0;                                                         \
  }                                                                                                              \
  extern "C" int fourier_hip_nufft3d_set_points_##SUFFIX(fc::fourier_nufft3d_##SUFFIX* h, const double* h_x1, const double* h_x2, \
                                                         const double* h_x3, size_t m, void* stream) {           \
    Nufft3dPlan<T>* p = (Nufft3dPlan<T>*)h;                                                                      \
    return guarded_handle(p, [&] { p->set_points(h_x1, h_x2, h_x3, m, (hipStream_t)stream); });                  \
  }                                                                                                              \
  extern "C" int fourier_hip_nufft3d_to_modes_batch_##SUFFIX(const fc::fourier_nufft3d_##SUFFIX* h, const void* d_in, void* d_out, \
                                                             size_t batch, int sign, int order, void* stream) {  \
    const Nufft3dPlan<T>* p = (const Nufft3dPlan<T>*)h;                                                          \
    return guarded_handle(p, [&] { p->to_modes(d_in, d_out, batch, sign, order, (hipStream_t)stream); });        \
  }                                                                                                              \
  extern "C" int fourier_hip_nufft3d_to_points_batch_##SUFFIX(const fc::fourier_nufft3d_##SUFFIX* h, const void* d_in, void* d_out, \
                                                              size_t batch, int sign, int order, void* stream) { \
    const Nufft3dPlan<T>* p = (const Nufft3dPlan<T>*)h;                                                          \
    return guarded_handle(p, [&] { p->to_points(d_in, d_out, batch, sign, order, (hipStream_t)stream); });       \
  }                                                                                                              \
  extern "C" int fourier_hip_nufft3d_set_option_##SUFFIX(fc::fourier_nufft3d_##SUFFIX* h, const char* key, long long v) { \
    return set_handle_option<Nufft3dPlan<T>>(h, key, v);                                                         \
  }

FOURIER_DEFINE_NUFFT3D_ABI(float, float)
FOURIER_DEFINE_NUFFT3D_ABI(double, double)

// ---- library-wide defaults for plans created afterwards
namespace fourier_hip {
namespace {
std::atomic<int> g_specialise_policy{-1};  // -1: not decided yet (the environment is read on first use)
}
int specialise_policy() {
  int v = g_specialise_policy.load(std::memory_order_relaxed);
  if (v < 0) {
    const char* e = getenv("FOURIER_HIP_SPECIALISE");  // "0", "1", "2": for programs that cannot be changed to call the function
    v = (e && *e >= '0' && *e <= '2' && !e[1]) ? *e - '0' : 1;
    g_specialise_policy.store(v, std::memory_order_relaxed);
  }
  return v;
}
void set_specialise_policy(int v) { g_specialise_policy.store(v, std::memory_order_relaxed); }
namespace {
std::atomic<int> g_register_stages{-1};
}
int register_stages_default() {
  int v = g_register_stages.load(std::memory_order_relaxed);
  if (v < 0) {
    const char* e = getenv("FOURIER_HIP_REGISTER_STAGES");
    v = (e && e[0] == '1' && !e[1]) ? 1 : 0;
    g_register_stages.store(v, std::memory_order_relaxed);
  }
  return v;
}
void set_register_stages_default(int v) { g_register_stages.store(v, std::memory_order_relaxed); }
}  // namespace fourier_hip

extern "C" int fourier_hip_set_default_option(const char* key, long long v) {
  if (!key) return fc::FOURIER_HIP_INVALID_ARGUMENT;
  if (std::string(key) == "specialise_at_create" && v >= 0 && v <= 2) { set_specialise_policy((int)v); return fc::FOURIER_HIP_OK; }
  if (std::string(key) == "register_stages_at_create" && (v == 0 || v == 1)) { set_register_stages_default((int)v); return fc::FOURIER_HIP_OK; }
  return fc::FOURIER_HIP_INVALID_ARGUMENT;
}
extern "C" long long fourier_hip_get_default_option(const char* key) {
  if (key && std::string(key) == "specialise_at_create") return specialise_policy();
  if (key && std::string(key) == "register_stages_at_create") return register_stages_default();
  return -1;
}

extern "C" const char* fourier_hip_status_string(int status) {
  switch (status) {
    case fc::FOURIER_HIP_OK: return "ok";
    case fc::FOURIER_HIP_INVALID_ARGUMENT: return "invalid argument";
    case fc::FOURIER_HIP_OUT_OF_MEMORY: return "out of device memory";
    case fc::FOURIER_HIP_RUNTIME_ERROR: return "HIP runtime error";
    case fc::FOURIER_HIP_UNSUPPORTED: return "unsupported size";
    default: return "unknown status";
  }
}

#ifdef FOURIER_EMU
// test-only: LDS bank-conflict statistics gathered by the emulator
extern "C" void fourier_emu_lds_stats(uint64_t* instr, uint64_t* cycles, uint64_t* ideal, int reset) {
  auto& s = hipemu::lds_stats();
  *instr = s.instr; *cycles = s.cycles; *ideal = s.ideal;
  if (reset) { s.instr = 0; s.cycles = 0; s.ideal = 0; }
}
// test-only: number of device allocations so far (tests/test_engine_emu.py: reserve makes calls allocation-free)
extern "C" uint64_t fourier_emu_alloc_count() { return hipemu::alloc_count(); }
#endif
