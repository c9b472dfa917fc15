// bandspec_plan.h -- the plan behind a band-energy spectrogram handle (fourier_hip_bandspec_*, include/fourier.h): of the STFT's frames
// X[b, f, k] the projection Y[b, f, j] = sum_k W[j, k] |X[b, f, k]|^p onto the rows of a real bands x bins matrix W (a mel, bark or
// third-octave bank, or any sparse-row matrix; negative weights allowed), optionally log_mult * ln(max(Y, log_floor)), frame-major
// batch x frames x bands reals, without |X|^p reaching memory the caller sees.  It owns a StftPlan<T> and takes from it the framing, the
// window table and the real plan, as SpectrogramPlan and CsdPlan do; the STFT's own routes are not touched.
// The bank (set_bands): row j is kept as its support [lo_j, hi_j) -- first non-zero column to last non-zero column + 1, zeros inside
// kept -- and the weights of that run; an all-zero row has an empty run.  A band's sum runs in ascending k in ONE accumulator of type T.
// Routes, both chunked over the flat frame index:
//   "bandspec fused rows"  wherever stft_rows_kernel exists and bands <= bins: bandspec_rows_kernel (kernels_bandspec.h), one launch
//                          per LAUNCH_ITEMS frames, no scratch.
//   "bandspec composed"    every n_fft: per chunk stft_frame_kernel gathers, pads and windows into the scratch, RealPlan::run_forward
//                          transforms into a second region of it (FrameScratch, the spectrogram's walk), then bandspec_sweep_kernel,
//                          one lane per (frame, band), writes the caller's output.  Chunks may end inside a row.
// The default route follows the measurement at the constructor; option "fusion" = 1 takes the fused route wherever it exists, 0 the
// composed one.  No atomics and no sum across frames: equal calls give bit-equal results, under any scratch bound.
#pragma once
#include <cmath>

#include "frame_scratch.h"

namespace fourier_hip {

template <typename T> class BandSpecPlan : public HandleBase {
 public:
  static constexpr size_t LAUNCH_ITEMS = StftPlan<T>::LAUNCH_ITEMS;  // frames of one launch: 32-bit frame arithmetic in the kernels
  static constexpr size_t MAX_BANDS = 65535;

  BandSpecPlan(size_t n_fft, size_t hop, size_t win_length, int pad_mode, size_t bands, int device) : bands_(bands) {
    if (bands == 0 || bands > MAX_BANDS) throw EngineError(::fourier::c::FOURIER_HIP_INVALID_ARGUMENT, "1 <= bands <= 65535");
    stft_.reset(new StftPlan<T>(n_fft, hop, win_length, pad_mode, device));
    device_ = stft_->real().inner().device();
    DeviceGuard g(device_);
    frames_.cap = scratch_bound("FOURIER_REAL_SCRATCH_BYTES", REAL_SCRATCH_BYTES);
    launch_items_ = frames_.items = launch_bound("FOURIER_LAUNCH_ITEMS", LAUNCH_ITEMS);
    // Where the fused route is the default: wherever its kernels exist and bands <= bins.  The project's rule is that a default follows
    // a measurement: at 64 rows of 2^20 reals, (n_fft, hop, mels) = (512, 128, 40), (1024, 256, 80), (2048, 512, 128), the fused route
    // took 0.18 - 0.20 of the composed route's time at all five shapes where it exists (f32 0.40 - 0.44 ms against 2.14 - 2.34 ms, f64
    // 0.74 - 0.80 against 3.87 - 4.14 ms), against spreads of 0.2 - 6.1 % (tools/bandspec_bench.py; profiles/bandspec/bandspec_bench.jsonl;
    // DESIGN.md section 4, "Band-energy (mel) spectrogram").
    // FOURIER_BANDSPEC_FUSION = 0 / 1 is the development switch of the experiments library and the emulator build.
    fusion_.init(stft_->enable_bandspec() && bands_ <= bins(), "FOURIER_BANDSPEC_FUSION", FUSED_BY_DEFAULT);
    refresh_desc();
  }

  size_t n_fft() const { return stft_->n_fft(); }
  size_t hop() const { return stft_->hop(); }
  size_t win_length() const { return stft_->win_length(); }
  size_t bins() const { return stft_->bins(); }
  size_t bands() const { return bands_; }
  size_t frames(size_t length) const { return stft_->frames(length); }

  int set_option(const std::string& key, long long v) {
    if (!fusion_.set(key, v)) return ::fourier::c::FOURIER_HIP_INVALID_ARGUMENT;
    refresh_desc();
    return ::fourier::c::FOURIER_HIP_OK;
  }

  // the STFT handle's set-up call: win_length reals T on the device, or nullptr for all ones; waits for `stream`
  void set_window(const void* d_window, hipStream_t stream) { stft_->set_window(d_window, stream); }

  // bands x bins reals T, row-major, on the HOST.  A set-up call: it waits for `stream` before the bank in use is replaced and again
  // after the upload.  The supports are found here; a weight that is NaN or infinite refuses the call and leaves the bank as it was.
  void set_bands(const void* h_matrix, hipStream_t stream) {
    const int INVALID = ::fourier::c::FOURIER_HIP_INVALID_ARGUMENT;
    if (!h_matrix) throw EngineError(INVALID, "null matrix");
    if ((uintptr_t)h_matrix % sizeof(T)) throw EngineError(INVALID, "misaligned matrix");
    const T* m = (const T*)h_matrix;
    const size_t nb = bins();
    if (bands_ * nb > 0xffffffffull) throw EngineError(::fourier::c::FOURIER_HIP_UNSUPPORTED, "bands * bins above 2^32");
    std::vector<uint32_t> lo(bands_), off(bands_ + 1);
    std::vector<T> w;
    for (size_t j = 0; j < bands_; ++j) {
      const T* row = m + j * nb;
      size_t first = nb, last = 0;
      for (size_t k = 0; k < nb; ++k) {
        if (!std::isfinite(row[k])) throw EngineError(INVALID, "a band weight is NaN or infinite");
        if (row[k] != (T)0) { if (first == nb) first = k; last = k + 1; }
      }
      off[j] = (uint32_t)w.size();
      lo[j] = first == nb ? 0 : (uint32_t)first;
      if (first != nb) w.insert(w.end(), row + first, row + last);
    }
    off[bands_] = (uint32_t)w.size();
    if (w.empty()) w.push_back((T)0);  // an all-zero bank: a table nobody reads
    DeviceGuard g(device_);
    HIP_CHECK(hipStreamSynchronize(stream));
    lo_.upload(lo);
    off_.upload(off);
    w_.upload(w);
    HIP_CHECK(hipStreamSynchronize(stream));
    have_bank_ = true;
  }

  // later forward calls of at most `batch` rows of `length` reals never allocate (on the route selected now); the bank's buffers
  // belong to set_bands
  void reserve(size_t length, size_t batch) const {
    const size_t fr = frames(length);
    if (fr == 0) throw EngineError(::fourier::c::FOURIER_HIP_INVALID_ARGUMENT, "invalid length");
    if (batch == 0) return;
    DeviceGuard g(device_);
    if (!fusion_.on) (void)frames_.prepare(*stft_, batch * fr);
  }

  void forward(const void* d_in, void* d_out, size_t length, size_t batch, int power, bool normalized, double log_mult, double log_floor,
               hipStream_t stream) const {
    const int INVALID = ::fourier::c::FOURIER_HIP_INVALID_ARGUMENT;
    if (power != ::fourier::c::FOURIER_SPECTROGRAM_MAGNITUDE && power != ::fourier::c::FOURIER_SPECTROGRAM_POWER)
      throw EngineError(INVALID, "power must be 1 (magnitude) or 2 (power)");
    if (!std::isfinite(log_mult)) throw EngineError(INVALID, "log_mult must be finite");
    if (log_mult != 0 && !(std::isfinite(log_floor) && log_floor > 0 && (double)(T)log_floor > 0 && std::isfinite((T)log_floor)))
      throw EngineError(INVALID, "log_floor must be finite and > 0");
    if (!have_bank_) throw EngineError(INVALID, "no bank: call set_bands first");
    const size_t fr = frames(length), bins = this->bins();
    if (fr == 0) throw EngineError(INVALID, "invalid length");
    check_buffers(d_in, d_out, batch * length * sizeof(T), batch * fr * bands_ * sizeof(T), sizeof(T), false);
    if (batch == 0) return;
    DeviceGuard g(device_);
    const size_t total = batch * fr;
    const T* in = (const T*)d_in;
    T* out = (T*)d_out;
    BandSpecArgs a{};
    a.f = fusion_.on ? stft_->fused_args(length, fr, normalized) : stft_->frame_args(length, fr);
    a.lo = lo_.p; a.off = off_.p; a.w = w_.p;
    a.bins = (uint32_t)bins; a.bands = (uint32_t)bands_;
    a.power = (uint32_t)power;
    a.log_mult = log_mult; a.log_floor = log_mult != 0 ? log_floor : 0.0;
    if (fusion_.on) {
      for_chunks(total, launch_items_, [&](size_t g0, size_t ng) {
        stft_->fused_launch_at(a.f, in, length, fr, g0, ng);
        a.f.out = out + g0 * bands_;
        stft_->real().inner().exec_frames(a, stream, power);
      });
      return;
    }
    const size_t chunk = frames_.prepare(*stft_, total);
    const int code = normalized ? ::fourier::c::FOURIER_TRANSFORM_SQRT_SCALED_FFT : ::fourier::c::FOURIER_TRANSFORM_FFT;
    const StftArgs block = a.f;
    for_chunks(total, chunk, [&](size_t g0, size_t ng) {
      frames_.transform_chunk(*stft_, block, in, length, fr, g0, ng, chunk, code, stream);
      a.f.in = frames_.spectra();
      a.f.out = out + g0 * bands_;
      a.count = ng * bands_;
      FOURIER_LAUNCH(get_bandspec_kernel(Real<T>{}), elementwise_grid(a.count), 256, 0, stream, a);
    });
  }

 private:
  // The measured default (the constructor's comment).
  static constexpr bool FUSED_BY_DEFAULT = true;

  void refresh_desc() { desc_ = std::string(fusion_.on ? "bandspec fused rows: " : "bandspec composed: ") + stft_->real().describe(); }

  size_t bands_;
  std::unique_ptr<StftPlan<T>> stft_;
  int device_ = 0;
  FusionSwitch fusion_;
  size_t launch_items_ = LAUNCH_ITEMS;  // frames of one launch (development switch FOURIER_LAUNCH_ITEMS)
  FrameScratch<T> frames_;
  DevBuf lo_, off_, w_;
  bool have_bank_ = false;
};

}  // namespace fourier_hip
